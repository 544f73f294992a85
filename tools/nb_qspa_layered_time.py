"""What the layered schedule of the FHT sum-product decoder (nbldpc_qspa_layered_decode_batch, k_nb_qspa_layered) costs next to the
flooding one (nbldpc_qspa_decode_batch, k_nb_qspa), one session on one card.  The codes and the batch of tools/nb_qspa_time.py:
BDS.576.288.GF.64 and LDPC_N96_K48_GF256_d1_exp, random codewords over BPSK from the device channel.

Part 1, per iteration: an Eb/N0 so low that no frame converges, so that both schedules run their 20 iterations on every frame (the ok
counts are printed: 0 is what the per-iteration figures assume).  Part 2, a whole decode on BDS.576.288.GF.64 at 2.0 and 3.0 dB, where
the schedules stop at different iteration counts: this is the figure that says which schedule decodes a frame faster.
Whole calls of the C ABI between HIP events on the stream after warm-up, outputs preallocated, flooding and layered alternating inside
every repetition; median [min .. max].  The workgroup size of the layered kernel is the code object's (the rule of include/nbldpc.h,
or NBLDPC_QSPA_LAYERED_THREADS).
usage: python tools/nb_qspa_layered_time.py [--reps R] [--batch B] [--snr DB] [--out FILE]   (GPU box)"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cuda_ldpc_amd import nbldpc as nb  # noqa: E402
from cuda_ldpc_amd._lib import lib  # noqa: E402
from harq_time import timed_round  # noqa: E402

MAXIT = 20
LABEL = {"flood": "flooding (method 4)", "layer": "layered (method 5)"}


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, lib.nbldpc_last_error().decode(errors="replace")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--snr", type=float, default=-2.0, help="Eb/N0 of part 1: low enough that nothing converges")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("at least 7 repetitions")
    if not torch.cuda.is_available():
        sys.exit("nb_qspa_layered_time.py needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# python tools/nb_qspa_layered_time.py --reps %d --batch %d --snr %g" % (args.reps, args.batch, args.snr))
    emit("# %s, %d repetitions, C-ABI calls on preallocated outputs, alternating; maxIT = %d; ms = median [min .. max]; "
         "ns / frame-iteration = ms / (frames * iterations run)" % (torch.cuda.get_device_name(0), args.reps, MAXIT))
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nbd = os.path.join(ROOT, "data", "nb")
    B = args.batch

    def measure(code, snr, per_iteration):
        sigma = nb.sigma_of(snr, code.rate)
        words = nb.PN_CodeWords(code, 1, B)
        Lch = nb.Demodulate(code, nb.AWGNChannel_GPU(np.array([173, 173, 173], np.int32), sigma, code, words, B), sigma)
        dec = {k: [torch.empty((B, code.N), dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"),
                   torch.empty(B, dtype=torch.int32, device="cuda")] for k in LABEL}
        calls = {"flood": lib.nbldpc_qspa_decode_batch, "layer": lib.nbldpc_qspa_layered_decode_batch}

        def run(k):
            d = dec[k]
            check(calls[k](code._h, P(Lch), B, MAXIT, P(d[0]), P(d[1]), P(d[2]), None, None, st), LABEL[k])

        fns = {k: (lambda k=k: run(k)) for k in LABEL}
        kern = {}
        for k, f in fns.items():
            for _ in range(2):
                f()
            kern[k] = code.last_kernel
        torch.cuda.synchronize()
        t = timed_round(fns, args.reps)
        emit("# Eb/N0 %g dB (sigma %.4f); B = %d frames; k_nb_qspa_layered with %d threads per workgroup (k_nb_qspa: 1024)"
             % (snr, sigma, B, code.qspa_layered_threads))
        emit("# %-22s %-20s %28s %14s %8s %8s %10s %22s" % ("schedule", "kernel", "ms", "codewords/s", "ok", "errors", "mean it", "ns / frame-iteration"))
        med, per_it = {}, {}
        for k in LABEL:
            med[k] = float(np.median(t[k]))
            its = dec[k][1].long() + dec[k][2].long()  # a frame that stopped ran one iteration more than it reports
            per_it[k] = med[k] * 1e6 / float(its.sum())
            bad = int((dec[k][0] != words).any(dim=1).sum())
            emit("  %-22s %-20s %8.3f [%8.3f .. %8.3f] %14.0f %8d %8d %10.3f %22.1f" % (LABEL[k], kern[k], med[k], min(t[k]), max(t[k]), B / med[k] * 1e3,
                                                                                      int(dec[k][2].sum()), bad, float(dec[k][1].float().mean()), per_it[k]))
        if per_iteration:
            emit("  one layered iteration costs %.3f flooding iterations" % (per_it["layer"] / per_it["flood"]))
        else:
            emit("  a layered decode takes %.3f of the time of a flooding decode (%s is faster)"
                 % (med["layer"] / med["flood"], "layered" if med["layer"] < med["flood"] else "flooding"))

    for name in ("BDS.576.288.GF.64", "LDPC_N96_K48_GF256_d1_exp"):
        H = nb.NBMatrix(os.path.join(nbd, name + ".txt"))
        mul, _, _ = nb.GFInitial(H.q, os.path.join(nbd, "GF", "Arith.Table.GF.%d.txt" % H.q))
        code = nb.NBCode(os.path.join(nbd, name + ".txt"), mul)
        emit("# %s N=%d q=%d dc=%d, %d row levels" % (name, code.N, code.q, code.dc, _levels(code)))
        emit("# part 1: per iteration")
        measure(code, args.snr, True)
        if name.startswith("BDS"):
            emit("# part 2: a whole decode")
            for snr in (2.0, 3.0):
                measure(code, snr, False)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def _levels(code):
    """The row dependency levels of the code, restated: 1 + the highest level among the earlier rows that share a variable."""
    last, top = {}, 0
    for r in range(code.M):
        cols = [int(c) for c in code.cn_linkVNs[r, :code.cn_weight[r]]]
        lv = max(last.get(c, -1) for c in cols) + 1
        for c in cols:
            last[c] = lv
        top = max(top, lv + 1)
    return top


if __name__ == "__main__":
    main()
