"""What the workspace tier of the FHT sum-product decoders (nbldpc_qspa_ws_decode_batch: k_nb_qspa_ws, k_nb_qspa_ws_layered) costs,
one session on one card:
  (a) Tanner_74_9_Z128_GF16, flooding and layered, next to EMS(2,2) on k_nb_ems_hbm on the same input;
  (b) LDPC_N576_K480_GF256_exp, likewise;
  (c) BDS.576.288.GF.64 with the workspace tier forced, next to the LDS tier (k_nb_qspa, k_nb_qspa_layered): the price of the
      workspace, which tier="auto" never pays;
  (d) every workgroup size that fits on (a) and (b), through the pin NBLDPC_QSPA_WS_THREADS (one code object per size).
The all-zero codeword over BPSK from the device channel at an Eb/N0 so low that no frame converges, so that every decoder runs its
maxIT iterations on every frame (the ok counts are printed: 0 is what the per-iteration figures assume).  Whole calls of the C ABI
between HIP events on the stream after warm-up, outputs preallocated, the variants of a group alternating inside every repetition;
median [min .. max].
usage: python tools/nb_qspa_ws_time.py [--reps R] [--snr DB] [--maxit I] [--b-tanner B] [--b-gf256 B] [--b-bds B] [--out FILE]   (GPU box)"""
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

SIZES = (64, 128, 256, 512, 1024)
PIN = "NBLDPC_QSPA_WS_THREADS"


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, lib.nbldpc_last_error().decode(errors="replace")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--snr", type=float, default=-2.0, help="Eb/N0 of the input: low enough that nothing converges")
    ap.add_argument("--maxit", type=int, default=10)
    ap.add_argument("--b-tanner", type=int, default=256)
    ap.add_argument("--b-gf256", type=int, default=4096)
    ap.add_argument("--b-bds", type=int, default=8192)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("at least 7 repetitions")
    if not torch.cuda.is_available():
        sys.exit("nb_qspa_ws_time.py needs a GPU")
    if PIN in os.environ:
        sys.exit("unset %s: the tool pins the sizes itself" % PIN)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# python tools/nb_qspa_ws_time.py --reps %d --snr %g --maxit %d --b-tanner %d --b-gf256 %d --b-bds %d"
         % (args.reps, args.snr, args.maxit, args.b_tanner, args.b_gf256, args.b_bds))
    emit("# %s, %d repetitions, C-ABI calls on preallocated outputs, the variants of a group alternating; maxIT = %d; ms = median [min .. max]; "
         "ns / frame-iteration = ms / (frames * iterations run)" % (torch.cuda.get_device_name(0), args.reps, args.maxit))
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nbd = os.path.join(ROOT, "data", "nb")

    def make_code(name, q, threads=None):
        mul, _, _ = nb.GFInitial(q, os.path.join(nbd, "GF", "Arith.Table.GF.%d.txt" % q))
        if threads is not None:
            os.environ[PIN] = str(threads)
        try:
            return nb.NBCode(os.path.join(nbd, name + ".txt"), mul)
        finally:
            os.environ.pop(PIN, None)

    def group(title, code, Lch, variants, base):
        """variants: [(label, code object, call)], call one of ("ws", layered) | ("lds", layered) | ("ems",).  base: the label the
        last column is relative to."""
        B = Lch.shape[0]
        outs, fns, codes = {}, {}, {}
        for label, c, call in variants:
            d = outs[label] = [torch.empty((B, c.N), dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"),
                               torch.empty(B, dtype=torch.int32, device="cuda")]
            if call[0] == "ws":
                fns[label] = lambda c=c, d=d, lay=call[1]: check(lib.nbldpc_qspa_ws_decode_batch(
                    c._h, P(Lch), B, lay, args.maxit, P(d[0]), P(d[1]), P(d[2]), None, None, st), "workspace tier")
            elif call[0] == "lds":
                f = lib.nbldpc_qspa_layered_decode_batch if call[1] else lib.nbldpc_qspa_decode_batch
                fns[label] = lambda c=c, d=d, f=f: check(f(c._h, P(Lch), B, args.maxit, P(d[0]), P(d[1]), P(d[2]), None, None, st), "LDS tier")
            else:
                fns[label] = lambda c=c, d=d: check(lib.nbldpc_ems_decode_batch(
                    c._h, P(Lch), B, 2, 2, args.maxit, 0, P(d[0]), P(d[1]), P(d[2]), None, None, st), "EMS(2,2)")
            codes[label] = c
        kern = {}
        for label, f in fns.items():  # warm-up, and the kernel's name
            f()
            f()
            kern[label] = codes[label].last_kernel
        torch.cuda.synchronize()
        t = timed_round(fns, args.reps)
        emit("# " + title)
        emit("# %-34s %-24s %7s %7s %30s %12s %6s %22s %10s" % ("variant", "kernel", "threads", "frames", "ms", "codewords/s", "ok",
                                                                 "ns / frame-iteration", "x " + base))
        med = {k: float(np.median(v)) for k, v in t.items()}
        for label, c, call in variants:
            d = outs[label]
            its = d[1].long() + d[2].long()  # a frame that stopped ran one iteration more than it reports
            threads = "-" if call[0] != "ws" else str(c.qspa_ws_info(bool(call[1]))["threads"])
            emit("  %-34s %-24s %7s %7d %9.3f [%8.3f .. %8.3f] %12.0f %6d %22.1f %10.2f" % (
                label, kern[label], threads, B, med[label], min(t[label]), max(t[label]), B / med[label] * 1e3, int(d[2].sum()),
                med[label] * 1e6 / float(its.sum()), med[label] / med[base]))

    def inputs(code, B):
        sigma = nb.sigma_of(args.snr, code.rate)
        zero = torch.zeros(code.N, dtype=torch.int32, device="cuda")
        return nb.Demodulate(code, nb.AWGNChannel_GPU(np.array([173, 173, 173], np.int32), sigma, code, zero, B), sigma)

    for tag, name, q, B in (("a", "Tanner_74_9_Z128_GF16", 16, args.b_tanner), ("b", "LDPC_N576_K480_GF256_exp", 256, args.b_gf256)):
        code = make_code(name, q)
        Lch = inputs(code, B)
        head = "%s N=%d q=%d dc=%d, Eb/N0 %g dB, B = %d" % (name, code.N, code.q, code.dc, args.snr, B)
        group("(%s) %s: the workspace tier next to EMS(2,2)" % (tag, head), code, Lch,
              [("sum-product, workspace", code, ("ws", 0)), ("layered sum-product, workspace", code, ("ws", 1)), ("EMS(2,2)", code, ("ems",))],
              "EMS(2,2)")
        for lay, word in ((0, "flooding"), (1, "layered")):
            rule = code.qspa_ws_info(bool(lay))["threads"]
            pinned = []
            for nt in SIZES:
                try:
                    c = make_code(name, q, nt)
                    c.qspa_ws_info(bool(lay))
                    pinned.append(("%s, %d threads%s" % (word, nt, " (the rule)" if nt == rule else ""), c, ("ws", lay)))
                except nb.LdpcError:
                    emit("# (d) %s, %s: %d threads do not fit" % (name, word, nt))
            base = next(label for label, _, _ in pinned if label.endswith("(the rule)"))
            group("(d) %s, %s: the workgroup sizes that fit, pinned" % (head, word), code, Lch, pinned, base)
        del Lch
    code = make_code("BDS.576.288.GF.64", 64)
    Lch = inputs(code, args.b_bds)
    for lay, word in ((0, "sum-product"), (1, "layered sum-product")):
        group("(c) BDS.576.288.GF.64 N=%d q=64 dc=%d, Eb/N0 %g dB, B = %d, %s: the workspace tier forced on a code the LDS tier takes"
              % (code.N, code.dc, args.snr, args.b_bds, word), code, Lch,
              [(word + ", LDS", code, ("lds", lay)), (word + ", workspace", code, ("ws", lay))], word + ", LDS")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
