"""What the rate-matched channel costs next to the calls it replaces, one session on one card, the all-zero word:
  fused        bldpc_rm_awgn_channel_device            one kernel writes the decoder's [N][F] input, noise for the E transmitted bits
  two calls    bldpc_awgn_channel_device with N := E, then bldpc_rm_recover     an [E][F] intermediate and a second pass
  plain        bldpc_awgn_channel_device at N          the mother code's channel; scaled by E / N it is what the fused call should cost
on J4_L24_Z96 with 65 536 frames and PON_LDPC (J12_L69_Z256) with 4 096, about 1 % of the positions shortened (the head of the
information part) and 3 % punctured (a range in the parity part).  Whole calls of the C ABI between HIP events on the stream after
warm-up, every output preallocated (no call allocates), the variants alternating inside every repetition; median [min .. max].
usage: python tools/rm_time.py [--reps R] [--out FILE]   (GPU box)"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cuda_ldpc_amd as C  # noqa: E402
from cuda_ldpc_amd._lib import check, lib  # noqa: E402


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
    if args.reps < 7:
        ap.error("at least 7 repetitions")
    if not torch.cuda.is_available():
        sys.exit("rm_time.py needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# %s, %d repetitions, C-ABI calls on preallocated outputs, alternating, all-zero word; ms = median [min .. max]" % (
        torch.cuda.get_device_name(0), args.reps))
    emit("# %-12s %-44s %24s %10s" % ("code", "call", "ms", "GB/s out"))
    for name, L, Z, F in (("J4_L24_Z96", 24, 96, 65536), ("PON_LDPC", 69, 256, 4096)):
        N = L * Z
        rm = C.RateMatch(N, range(0, N // 100), range(N - Z // 4 - 3 * N // 100, N - Z // 4))
        E = rm.E
        sigma, llr = ctypes.c_float(0.7), ctypes.c_float(1.0e4)
        y = torch.empty((N, F), device="cuda")
        y2 = torch.empty((N, F), device="cuda")
        yN = torch.empty((N, F), device="cuda")
        rx = torch.empty((E, F), device="cuda")
        seed = np.array([173, 173, 173], np.int32)
        sp = seed.ctypes.data_as(ctypes.c_void_p)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

        def two_calls():
            check(lib.bldpc_awgn_channel_device(sp, sigma, P(rx), None, E, F, st), "channel at E")
            check(lib.bldpc_rm_recover(rm._h, P(rx), F, llr, P(y2), st), "recover")

        fns = {
            "fused (bldpc_rm_awgn_channel_device)": lambda: check(lib.bldpc_rm_awgn_channel_device(rm._h, sp, sigma, None, F, llr, P(y), st), "fused"),
            "two calls (channel at E, bldpc_rm_recover)": two_calls,
            "plain (bldpc_awgn_channel_device at N)": lambda: check(lib.bldpc_awgn_channel_device(sp, sigma, P(yN), None, N, F, st), "plain"),
        }
        for f in fns.values():
            for _ in range(2):
                f()
        torch.cuda.synchronize()
        t = timed_round(fns, args.reps)
        med = {k: float(np.median(v)) for k, v in t.items()}
        for k in fns:
            emit("  %-12s %-44s %8.3f [%6.3f .. %6.3f] %10.1f" % (name, k, med[k], min(t[k]), max(t[k]), 4 * N * F / med[k] / 1e6))
        fused, two, plain = (med[k] for k in fns)
        emit("  %-12s N=%d E=%d F=%d n_short=%d n_punct=%d: fused / two calls = %.3f;  fused / (plain * E / N) = %.3f" % (
            name, N, E, F, rm.n_short, rm.n_punct, fused / two, fused / (plain * E / N)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
