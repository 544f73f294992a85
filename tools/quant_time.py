"""Quantised layered min-sum against fp32 layered min-sum decode rates, one session on one card, for the two bench.py codes at
bench.py's batch sizes (the codes and batches of tools/layered_time.py and tools/bp_time.py):
  (a) 25 fixed iterations: fp32 layered min-sum alpha 0.75 (LDPC_Decoder_Layered_GPU) and the quantised decoder
      (LDPC_Decoder_Quant_GPU, Quant(6, 8, 6, norm8=6, llr_scale=16)), with the time per frame and iteration and the ratio of the two
  (b) both per-frame paths at Es/N0 3.0, 3.6 and 4.2 dB (max 25, prefix rule -- the all-zero codeword is sent, as in bench.py), with the
      mean iteration count and the frames left unflagged.
Whole calls (input regrouping / quantising, kernel, unpacking of D) between HIP events on the stream, after warm-up; the two decoders
alternate inside every repetition; median, min and max over the repetitions are printed, the rate is frames / median.
usage: python tools/quant_time.py [--reps R] [--out FILE]   (GPU box)"""
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
FP32 = "fp32 layered min-sum alpha=0.75"
QUANT = "quantised layered (6,8,6) norm8=6"


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
        sys.exit("quant_time.py needs a GPU")
    lines = []
    q = C.Quant(6, 8, 6, norm8=6, offset=0, llr_scale=16.0)

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# %s, %d repetitions, decoders alternating; ms = median [min .. max] of whole calls; rate = frames / median; "
         "ns/(frame it) = median / (frames * meanIT); %r" % (torch.cuda.get_device_name(0), args.reps, q))
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
            med = {}
            for k in fns:
                fns[k]()
                kern = code.last_kernel
                it = mean_it()
                med[k] = float(np.median(t[k]))
                emit("  %-12s %6d %-36s %-10s %6.1f %9.3f [%6.3f .. %6.3f] %9.3f %7.2f %9d %13.2f" % (
                    name, F, k, kern, s, med[k], min(t[k]), max(t[k]), F / med[k] / 1e3, it, unfl(), med[k] * 1e6 / (F * it)))
            emit("# %s at %.1f dB: the quantised decoder decodes %.2f times the codewords per second of the fp32 one (whole calls)" % (
                name, s, med[FP32] / med[QUANT]))

        y = C.AWGNChannel_GPU(np.array([173, 173, 173], np.int32), C.sigma_of(snr), code.N, F)
        emit("# %d fixed iterations" % ITERS)
        run(snr, {FP32: lambda: C.LDPC_Decoder_Layered_GPU(code, y, max_iter=ITERS, alpha=0.75, D=D),
                  QUANT: lambda: C.LDPC_Decoder_Quant_GPU(code, y, q, max_iter=ITERS, D=D)}, lambda: float(ITERS))
        emit("# per-frame exit, at most %d iterations" % ITERS)
        for s in PF_SNR:
            y = C.AWGNChannel_GPU(np.array([173, 173, 173], np.int32), C.sigma_of(s), code.N, F)
            last = {}

            def lay():
                last["it"] = C.LDPC_Decoder_Layered_GPU(code, y, max_iter=ITERS, alpha=0.75, exit_mode=C.EXIT_PER_FRAME, D=D)["iters"]

            def quant():
                last["it"] = C.LDPC_Decoder_Quant_GPU(code, y, q, max_iter=ITERS, exit_mode=C.EXIT_PER_FRAME, D=D)["iters"]

            run(s, {FP32: lay, QUANT: quant}, lambda: float(last["it"].float().mean()))
        code.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
