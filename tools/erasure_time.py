"""Peeling decode times against the flooding min-sum decoder on the same erased words, one session on one card.
For J4_L24_Z96 and J32_L64_Z64 at 65 536 frames and PON at 4 096, on random codewords through the binary erasure channel at two erasure
rates each (one at which nearly every frame finishes, one above the threshold, where peeling stalls):
  (a) bldpc_decode_erasure with Dbits + Ebits, and with the int32 D as well; k_er leaves its loop once none of the 32 frames of a word
      makes progress, so the cap of 50 iterations is rarely reached;
  (b) what a user runs today for the same task: bldpc_decode_per_frame with the same cap on the +-1.0 / 0.0 floats of the same words,
      kernels this decoder leaves untouched.  Its exit rule tests for the all-zero word, so on random codewords it runs to the cap; the
      row "all-zero word" shows the same call on the all-zero word's floats, where every hard decision is 0 from the start and the rule
      stops a frame at once, whatever is still erased.
Then bldpc_bec_channel_device next to bldpc_bsc_channel_device, and bldpc_statistic_bits next to bldpc_hard_unpack +
bldpc_statistic_per_frame, at the same sizes.
Whole C-ABI calls between HIP events on the stream, outputs preallocated, after warm-up; the variants alternate inside every repetition;
median, min and max over the repetitions are printed.
usage: python tools/erasure_time.py [--reps R] [--out FILE]   (GPU box)"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cuda_ldpc_amd as C  # noqa: E402

lib = C._lib.lib
CODES = (  # file, J, L, Z, frames, erasure probabilities (below and above the peeling threshold)
    ("J4_L24_Z96_BlockH.txt", 4, 24, 96, 65536, (0.10, 0.16)),
    ("J32_L64_Z64_BlockH.txt", 32, 64, 64, 65536, (0.35, 0.50)),
    ("PON_LDPC.txt", 12, 69, 256, 4096, (0.10, 0.16)),
)
ITERS = 50


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def timed_round(fns, reps):
    """Every function once per repetition, in turn; returns {name: [ms per repetition]}."""
    out = {k: [] for k in fns}
    for _ in range(reps):
        ev = {}
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            ev[k] = (a, b)
        torch.cuda.synchronize()
        for k, (a, b) in ev.items():
            out[k].append(a.elapsed_time(b))
    return out


def popcount(t):
    return int(sum(bin(int(x) & 0xFFFFFFFF).count("1") for x in t.cpu().tolist()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("erasure_time.py needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def run(fns):
        for f in fns.values():  # warm-up: plans, scratch growth
            for _ in range(2):
                assert f() == 0
        torch.cuda.synchronize()
        t = timed_round(fns, args.reps)
        return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}

    emit("# %s, %d repetitions, variants alternating; ms = median [min .. max] of whole C-ABI calls between events; cap %d iterations"
         % (torch.cuda.get_device_name(0), args.reps, ITERS))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for fn, J, L, Z, F, ps in CODES:
        code = C.BinaryCode.from_blockh(os.path.join(ROOT, "data", "bldpc", fn), J, L, Z)
        name = fn.replace("_BlockH.txt", "").replace(".txt", "")
        N, W = code.N, (F + 31) // 32
        D = torch.empty((N + 1, F), dtype=torch.int32, device="cuda")
        Db = torch.empty((N + 1, W), dtype=torch.int32, device="cuda")
        Eb = torch.empty((N, W), dtype=torch.int32, device="cuda")
        it = torch.empty(F, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(5, dtype=torch.int64, device="cuda")
        cw = C.PN_CodeWords(code, 1, F)
        cwb = C.Hard_Pack_Int(cw)
        emit("# %s N=%d F=%d, k_er: %r" % (name, N, F, code.erasure_info()))
        emit("# %-14s %6s %-34s %-16s %24s %9s %11s %8s" % ("code", "p", "variant", "kernel", "ms", "Mcw/s", "unrecovered", "mean it"))
        for p in ps:
            bits, erased = C.BECChannel_GPU(np.array([173, 173, 173], np.int32), p, N, F, CodeWord=cw)
            known = 1.0 - C.Hard_Unpack(erased, F).float()
            y = ((1.0 - 2.0 * C.Hard_Unpack(bits, F).float()) * known).contiguous()  # +-1.0 where known, 0.0 where erased
            y0 = known.contiguous()  # the all-zero word through the same erasures

            def er(d, db, eb):
                return lambda: lib.bldpc_decode_erasure(code._h, ptr(bits), ptr(erased), F, ITERS, ptr(d), ptr(db), ptr(eb), ptr(it), st)

            def ms_pf(yy):
                return lambda: lib.bldpc_decode_per_frame(code._h, ptr(yy), F, ITERS, 0, C.KERNEL_AUTO, ptr(D), None, ptr(it), st)

            fns = {"peeling, Dbits + Ebits": er(None, Db, Eb), "peeling, Dbits + Ebits + D": er(D, Db, Eb),
                   "flooding min-sum per frame, D": ms_pf(y), "same, all-zero word": ms_pf(y0)}
            res = run(fns)
            for k, f in fns.items():
                assert f() == 0
                torch.cuda.synchronize()
                kern = code.last_kernel
                if "peeling" in k:
                    left = F - popcount(Db[N])
                else:  # by erasures the decoder could not fill: its soft value stays 0 there; count frames whose word differs from the one sent
                    ref = cw if "all-zero" not in k else torch.zeros_like(cw)
                    left = int(((D[:N] != ref).any(0)).sum())
                med, lo, hi = res[k]
                emit("  %-14s %6g %-34s %-16s %9.3f [%6.3f .. %6.3f] %9.3f %11d %8.2f" % (name, p, k, kern, med, lo, hi, F / med / 1e3, left,
                                                                                           float(it.float().mean())))
            ms = res["flooding min-sum per frame, D"][0]
            emit("# %s p=%g: time of the flooding min-sum call / time of the peeling call: %.2f (Dbits + Ebits) %.2f (with D)"
                 % (name, p, ms / res["peeling, Dbits + Ebits"][0], ms / res["peeling, Dbits + Ebits + D"][0]))
        # the channel next to the BSC, the packed statistics next to unpack + the int32 statistics (on the last decode's outputs)
        assert lib.bldpc_decode_erasure(code._h, ptr(bits), ptr(erased), F, ITERS, None, ptr(Db), ptr(Eb), ptr(it), st) == 0
        seed = np.array([173, 173, 173], np.int32)
        sp = seed.ctypes.data_as(ctypes.c_void_p)
        tmp, tmpe = torch.empty((N, W), dtype=torch.int32, device="cuda"), torch.empty((N, W), dtype=torch.int32, device="cuda")

        def unpack_stat():
            r = lib.bldpc_hard_unpack(ptr(Db), N + 1, F, ptr(D), st)
            return r or lib.bldpc_statistic_per_frame(code._h, ptr(D), ptr(cw), F, 0, ptr(it), ptr(cnt), st)

        fns = {"bldpc_bsc_channel_device": lambda: lib.bldpc_bsc_channel_device(sp, ctypes.c_float(0.1), ptr(cw), N, F, ptr(tmp), st),
               "bldpc_bec_channel_device": lambda: lib.bldpc_bec_channel_device(sp, ctypes.c_float(0.1), ptr(cw), N, F, ptr(tmp), ptr(tmpe), st),
               "bldpc_statistic_bits": lambda: lib.bldpc_statistic_bits(code._h, ptr(Db), ptr(Eb), ptr(cwb), F, 0, ptr(it), ptr(cnt), st),
               "unpack + bldpc_statistic_per_frame": unpack_stat}
        res = run(fns)
        for k in fns:
            med, lo, hi = res[k]
            emit("  %-14s %6s %-34s %-16s %9.3f [%6.3f .. %6.3f] %9.3f" % (name, "-", k, "-", med, lo, hi, F / med / 1e3))
        code.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
