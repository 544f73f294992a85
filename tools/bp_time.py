"""Layered sum-product against layered min-sum decode rates, one session on one card, for the two bench.py codes at bench.py's
batch sizes (the codes and batches of tools/layered_time.py):
  (a) 25 fixed iterations: layered min-sum alpha 0.75 (LDPC_Decoder_Layered_GPU) and sum-product (LDPC_Decoder_BP_GPU, llr_scale =
      2 / sigma^2), with the time per frame and iteration and the ratio of the two
  (b) both per-frame paths at Es/N0 3.0, 3.6 and 4.2 dB (max 25, prefix rule -- the all-zero codeword is sent, as in bench.py), with the
      mean iteration count and the frames left unflagged.
Whole calls (input regrouping, kernel, unpacking of D) between HIP events on the stream, after warm-up; the two decoders alternate
inside every repetition; median, min and max over the repetitions are printed, the rate is frames / median.
usage: python tools/bp_time.py [--reps R] [--out FILE]   (GPU box)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cuda_ldpc_amd as C  # noqa: E402

CODES = (  # file, J, L, Z, frames (bench.py), Es/N0 dB of the fixed-iteration workload (bench.py)
    ("J4_L24_Z96_BlockH.txt", 4, 24, 96, 65536, 3.0),
    ("J32_L64_Z64_BlockH.txt", 32, 64, 64, 32768, 0.0),
)
PF_SNR = (3.0, 3.6, 4.2)
ITERS = 25


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bp_time.py needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# %s, %d repetitions, decoders alternating; ms = median [min .. max] of whole calls; rate = frames / median; "
         "ns/(frame it) = median / (frames * meanIT)" % (torch.cuda.get_device_name(0), args.reps))
    emit("# %-12s %6s %-36s %-10s %6s %24s %9s %7s %9s %13s" % ("code", "F", "variant", "kernel", "Es/N0", "ms", "Mcw/s", "meanIT", "unflagged",
                                                             "ns/(frame it)"))
    for fn, J, L, Z, F, snr in CODES:
        code = C.BinaryCode.from_blockh(os.path.join(ROOT, "data", "bldpc", fn), J, L, Z)
        name = fn.replace("_BlockH.txt", "")
        D = torch.empty((code.N + 1, F), dtype=torch.int32, device="cuda")
        unfl = lambda: int((D[code.N] == 0).sum())  # noqa: E731

        def run(s, fns, mean_it):
            for f in fns.values():  # warm-up: plans, scratch growth
                for _ in range(2):
                    f()
            torch.cuda.synchronize()
            t = timed_round(fns, args.reps)
            per = {}
            for k in fns:
                fns[k]()
                kern = code.last_kernel
                it = mean_it()
                med = float(np.median(t[k]))
                per[k] = med * 1e6 / (F * it)
                emit("  %-12s %6d %-36s %-10s %6.1f %9.3f [%6.3f .. %6.3f] %9.3f %7.2f %9d %13.2f" % (
                    name, F, k, kern, s, med, min(t[k]), max(t[k]), F / med / 1e3, it, unfl(), per[k]))
            return per

        sigma = C.sigma_of(snr)
        y = C.AWGNChannel_GPU(np.array([173, 173, 173], np.int32), sigma, code.N, F)
        scale = 2.0 / (sigma * sigma)
        per = run(snr, {
            "layered min-sum 25 fixed alpha=0.75": lambda: C.LDPC_Decoder_Layered_GPU(code, y, max_iter=ITERS, alpha=0.75, D=D),
            "layered sum-product 25 fixed": lambda: C.LDPC_Decoder_BP_GPU(code, y, max_iter=ITERS, llr_scale=scale, D=D),
        }, lambda: float(ITERS))
        emit("# %s: a sum-product iteration costs %.2f min-sum iterations (whole calls, fixed %d iterations)" % (
            name, per["layered sum-product 25 fixed"] / per["layered min-sum 25 fixed alpha=0.75"], ITERS))
        for s in PF_SNR:
            sigma = C.sigma_of(s)
            y = C.AWGNChannel_GPU(np.array([173, 173, 173], np.int32), sigma, code.N, F)
            scale = 2.0 / (sigma * sigma)
            last = {}

            def lay():
                last["it"] = C.LDPC_Decoder_Layered_GPU(code, y, max_iter=ITERS, alpha=0.75, exit_mode=C.EXIT_PER_FRAME, D=D)["iters"]

            def bp():
                last["it"] = C.LDPC_Decoder_BP_GPU(code, y, max_iter=ITERS, llr_scale=scale, exit_mode=C.EXIT_PER_FRAME, D=D)["iters"]

            run(s, {"layered min-sum per-frame max 25 a=0.75": lay, "layered sum-product per-frame max 25": bp},
                lambda: float(last["it"].float().mean()))
        code.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
