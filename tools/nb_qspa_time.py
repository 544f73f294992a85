"""What the FHT sum-product decoder (nbldpc_qspa_decode_batch, k_nb_qspa) costs next to EMS(2,2) and to decoder_method 2
(log-QSPA = EMS(q, dc-1)), one session on one card.  BDS.576.288.GF.64 (N = 96 symbols of GF(64)) and LDPC_N96_K48_GF256_d1_exp
(N = 12 symbols of GF(256)); random codewords over BPSK from the device channel at an Eb/N0 so low that no frame converges, so that
every decoder runs its 20 iterations on every frame (the ok counts are printed: 0 is what the per-iteration figures assume).
Whole calls of the C ABI between HIP events on the stream after warm-up, outputs preallocated, sum-product and EMS(2,2) alternating
inside every repetition; median [min .. max].  Method 2 is orders of magnitude slower: it gets a batch of its own (--b2 frames) and
three timed calls after one warm-up, or that one call alone when it took more than --m2-limit seconds.
usage: python tools/nb_qspa_time.py [--reps R] [--batch B] [--b2 B2] [--snr DB] [--out FILE]   (GPU box)"""
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


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, lib.nbldpc_last_error().decode(errors="replace")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--b2", type=int, default=64, help="frames of the method-2 batch over GF(64); a quarter of it over GF(256)")
    ap.add_argument("--snr", type=float, default=-2.0, help="Eb/N0 of the input: low enough that nothing converges")
    ap.add_argument("--m2-limit", type=float, default=20.0, help="seconds: a method-2 warm-up call longer than this is the only one")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("at least 7 repetitions")
    if not torch.cuda.is_available():
        sys.exit("nb_qspa_time.py needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# python tools/nb_qspa_time.py --reps %d --batch %d --b2 %d --snr %g" % (args.reps, args.batch, args.b2, args.snr))
    emit("# %s, %d repetitions, C-ABI calls on preallocated outputs, alternating; maxIT = %d; ms = median [min .. max]; "
         "ns / frame-iteration = ms / (frames * iterations run)" % (torch.cuda.get_device_name(0), args.reps, MAXIT))
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nbd = os.path.join(ROOT, "data", "nb")
    for name, B2 in (("BDS.576.288.GF.64", args.b2), ("LDPC_N96_K48_GF256_d1_exp", max(args.b2 // 4, 1))):
        H = nb.NBMatrix(os.path.join(nbd, name + ".txt"))
        mul, _, _ = nb.GFInitial(H.q, os.path.join(nbd, "GF", "Arith.Table.GF.%d.txt" % H.q))
        code = nb.NBCode(os.path.join(nbd, name + ".txt"), mul)
        B = args.batch
        sigma = nb.sigma_of(args.snr, code.rate)
        words = nb.PN_CodeWords(code, 1, B)
        Lch = nb.Demodulate(code, nb.AWGNChannel_GPU(np.array([173, 173, 173], np.int32), sigma, code, words, B), sigma)
        dec = {k: [torch.empty((B, code.N), dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"),
                   torch.empty(B, dtype=torch.int32, device="cuda")] for k in ("qspa", "ems22", "m2")}

        def qspa():
            d = dec["qspa"]
            check(lib.nbldpc_qspa_decode_batch(code._h, P(Lch), B, MAXIT, P(d[0]), P(d[1]), P(d[2]), None, None, st), "sum-product")

        def ems22():
            d = dec["ems22"]
            check(lib.nbldpc_ems_decode_batch(code._h, P(Lch), B, 2, 2, MAXIT, 0, P(d[0]), P(d[1]), P(d[2]), None, None, st), "EMS(2,2)")

        def m2():
            d = dec["m2"]
            check(lib.nbldpc_ems_decode_batch(code._h, P(Lch), B2, code.q, code.dc - 1, MAXIT, 0, P(d[0]), P(d[1]), P(d[2]), None, None, st), "method 2")

        fns = {"qspa": qspa, "ems22": ems22}
        for f in fns.values():
            for _ in range(2):
                f()
        torch.cuda.synchronize()
        kern = {}
        qspa()
        kern["qspa"] = code.last_kernel
        ems22()
        kern["ems22"] = code.last_kernel
        torch.cuda.synchronize()
        t = timed_round(fns, args.reps)
        warm = timed_round({"m2": m2}, 1)["m2"]  # its first call is a measurement too: it may be the only one affordable
        kern["m2"] = code.last_kernel
        t["m2"] = warm if warm[0] > 1000.0 * args.m2_limit else timed_round({"m2": m2}, 3)["m2"]
        emit("# %s N=%d q=%d dc=%d, Eb/N0 %g dB (sigma %.4f); B = %d frames (method 2: %d)" % (name, code.N, code.q, code.dc, args.snr, sigma, B, B2))
        emit("# %-28s %-40s %7s %28s %14s %8s %22s" % ("decoder", "kernel", "frames", "ms", "codewords/s", "ok", "ns / frame-iteration"))
        per_it = {}
        for k, label, n in (("qspa", "FHT sum-product (method 4)", B), ("ems22", "EMS(2,2) (method 0)", B), ("m2", "EMS(q,dc-1) (method 2)", B2)):
            med = float(np.median(t[k]))
            its = dec[k][1][:n].long() + dec[k][2][:n].long()  # a frame that stopped ran one iteration more than it reports
            per_it[k] = med * 1e6 / float(its.sum())
            emit("  %-28s %-40s %7d %8.3f [%8.3f .. %8.3f] %14.0f %8d %22.1f" % (label, kern[k], n, med, min(t[k]), max(t[k]), n / med * 1e3,
                                                                                int(dec[k][2][:n].sum()), per_it[k]))
        emit("  one sum-product iteration costs %.2f EMS(2,2) iterations and %.5f method-2 iterations" % (per_it["qspa"] / per_it["ems22"],
                                                                                                      per_it["qspa"] / per_it["m2"]))
        del Lch, words, dec
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
