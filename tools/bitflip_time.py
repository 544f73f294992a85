"""Bit-flipping decode times against the flooding min-sum decoder, one session on one card.
For J4_L24_Z96 and J32_L64_Z64 at 65 536 frames and PON at 4 096, on the words of the binary symmetric channel at two crossover
probabilities each (one at which most frames converge, one at which hardly any does, so that every iteration runs: k_bf leaves its loop
once all 32 frames of a word are clean, in fixed mode too, with the same results):
  (a) 20 fixed iterations of each rule, bldpc_decode_bitflip with D (int32, 4 bytes per bit) and with Dbits only;
  (b) bldpc_decode with BLDPC_EXIT_FIXED, 20 iterations, on the +-1.0 values of the same words: kernels this decoder leaves untouched.
Then bldpc_bsc_channel_device and bldpc_hard_pack next to bldpc_awgn_channel_device at the same sizes.
Whole C-ABI calls between HIP events on the stream, outputs preallocated, after warm-up; the variants alternate inside every repetition;
median, min and max over the repetitions are printed.
usage: python tools/bitflip_time.py [--reps R] [--out FILE]   (GPU box)"""
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
CODES = (  # file, J, L, Z, frames, crossover probabilities
    ("J4_L24_Z96_BlockH.txt", 4, 24, 96, 65536, (0.004, 0.03)),
    ("J32_L64_Z64_BlockH.txt", 32, 64, 64, 65536, (0.02, 0.08)),
    ("PON_LDPC.txt", 12, 69, 256, 4096, (0.003, 0.03)),
)
ITERS = 20


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bitflip_time.py needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def run(fns):
        for f in fns.values():  # warm-up: plans, scratch growth
            for _ in range(2):
                f()
        torch.cuda.synchronize()
        t = timed_round(fns, args.reps)
        return {k: (float(np.median(v)), min(v), max(v)) for k, v in t.items()}

    emit("# %s, %d repetitions, variants alternating; ms = median [min .. max] of whole C-ABI calls between events; %d fixed iterations"
         % (torch.cuda.get_device_name(0), args.reps, ITERS))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for fn, J, L, Z, F, ps in CODES:
        code = C.BinaryCode.from_blockh(os.path.join(ROOT, "data", "bldpc", fn), J, L, Z)
        name = fn.replace("_BlockH.txt", "").replace(".txt", "")
        N, W = code.N, (F + 31) // 32
        D = torch.empty((N + 1, F), dtype=torch.int32, device="cuda")
        Db = torch.empty((N + 1, W), dtype=torch.int32, device="cuda")
        it = torch.empty(F, dtype=torch.int32, device="cuda")
        itera = ctypes.c_int(0)
        emit("# %s N=%d F=%d, k_bf: %r" % (name, N, F, code.bitflip_info()))
        emit("# %-14s %6s %-28s %-16s %24s %9s %10s %14s" % ("code", "p", "variant", "kernel", "ms", "Mcw/s", "unflagged", "ns/(frame it)"))
        for p in ps:
            bits = C.BSCChannel_GPU(np.array([173, 173, 173], np.int32), p, N, F)
            y = (1.0 - 2.0 * C.Hard_Unpack(bits, F).float()).contiguous()

            def bf(rule, d, db):
                return lambda: lib.bldpc_decode_bitflip(code._h, ptr(bits), F, ITERS, rule, C.EXIT_FIXED, ptr(d), ptr(db), ptr(it), st)

            fns = {"threshold, D": bf(C.BF_THRESHOLD, D, None), "threshold, Dbits only": bf(C.BF_THRESHOLD, None, Db),
                   "gradient, D": bf(C.BF_GRADIENT, D, None), "gradient, Dbits only": bf(C.BF_GRADIENT, None, Db),
                   "flooding min-sum, D": lambda: lib.bldpc_decode(code._h, ptr(y), F, ITERS, 0, C.EXIT_FIXED, C.KERNEL_AUTO, ptr(D), None, None,
                                                                   ctypes.byref(itera), st)}
            res = run(fns)
            for k, f in fns.items():
                assert f() == 0
                torch.cuda.synchronize()
                kern = code.last_kernel
                if "Dbits" in k:
                    unfl = F - int(sum(bin(int(x) & 0xFFFFFFFF).count("1") for x in Db[N].cpu().tolist()))
                elif "flooding" in k:  # its flag is the prefix rule on the word sent, which is not the all-zero word here: count by the syndrome
                    C.Syndrome(code, D, into_flag_row=True)
                    unfl = int((D[N] == 0).sum())
                else:
                    unfl = int((D[N] == 0).sum())
                med, lo, hi = res[k]
                emit("  %-14s %6g %-28s %-16s %9.3f [%6.3f .. %6.3f] %9.3f %10d %14.3f" % (name, p, k, kern, med, lo, hi, F / med / 1e3, unfl,
                                                                                     med * 1e6 / (F * ITERS)))
            ms = res["flooding min-sum, D"][0]
            emit("# %s p=%g: time of the flooding min-sum call / time of the bit-flip call: threshold %.2f (D) %.2f (Dbits only), "
                 "gradient %.2f (D) %.2f (Dbits only)" % (name, p, ms / res["threshold, D"][0], ms / res["threshold, Dbits only"][0],
                                                         ms / res["gradient, D"][0], ms / res["gradient, Dbits only"][0]))
        # the channel and the pack next to the AWGN channel
        yb = torch.empty((N, F), dtype=torch.float32, device="cuda")
        bits = torch.empty((N, W), dtype=torch.int32, device="cuda")
        seed = np.array([173, 173, 173], np.int32)
        sp = seed.ctypes.data_as(ctypes.c_void_p)
        fns = {"bldpc_awgn_channel_device": lambda: lib.bldpc_awgn_channel_device(sp, ctypes.c_float(0.5), ptr(yb), None, N, F, st),
               "bldpc_bsc_channel_device": lambda: lib.bldpc_bsc_channel_device(sp, ctypes.c_float(0.01), None, N, F, ptr(bits), st),
               "bldpc_hard_pack": lambda: lib.bldpc_hard_pack(ptr(yb), N, F, ptr(bits), st),
               "bldpc_hard_unpack": lambda: lib.bldpc_hard_unpack(ptr(bits), N, F, ptr(D), st)}
        res = run(fns)
        for k in fns:
            med, lo, hi = res[k]
            emit("  %-14s %6s %-28s %-16s %9.3f [%6.3f .. %6.3f] %9.3f" % (name, "-", k, "-", med, lo, hi, F / med / 1e3))
        code.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
