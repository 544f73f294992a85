"""What the HARQ calls cost, one session on one card, a codeword array of zeros (random codewords in (c)):
  (a) fused channel + combine (bldpc_rm_awgn_combine_device) against the three calls it replaces -- bldpc_rm_select,
      bldpc_awgn_channel_device at N := E, bldpc_rm_combine -- with E = Ncb and E = 2 Ncb, and with no frame done, the first half of the
      batch done (whole wavefronts) and every other frame done (scattered);
  (b) fused channel + combine at E = Ncb, no frame done, against bldpc_rm_awgn_channel_device on the linear profile of the same lists:
      the same number of samples, so the difference is the read-modify-write of the accumulator and the generality of the kernel;
  (c) one HARQ sweep point, Simulation_HARQ_GPU on J4_L24_Z96 at Es/N0 2.7 dB, compact=True against compact=False.
(a) and (b) on J4_L24_Z96 with 65 536 frames and PON_LDPC (J12_L69_Z256) with 4 096, about 1 % of the positions shortened and 3 %
punctured as in tools/rm_time.py.  Whole calls of the C ABI between HIP events on the stream after warm-up, every output preallocated,
the variants alternating inside every repetition; median [min .. max].
usage: python tools/harq_time.py [--reps R] [--out FILE]   (GPU box)"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cuda_ldpc_amd as C  # noqa: E402
from cuda_ldpc_amd._lib import check, lib  # noqa: E402
from cuda_ldpc_amd.simulation import HarqCounters, Simulation_HARQ_GPU  # noqa: E402


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
        sys.exit("harq_time.py needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# python tools/harq_time.py --reps %d" % args.reps)
    emit("# %s, %d repetitions, C-ABI calls on preallocated outputs, alternating, a codeword array of zeros; ms = median [min .. max]" % (
        torch.cuda.get_device_name(0), args.reps))
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sigma, llr = ctypes.c_float(0.7), ctypes.c_float(1.0e4)
    for name, L, Z, F in (("J4_L24_Z96", 24, 96, 65536), ("PON_LDPC", 69, 256, 4096)):
        N = L * Z
        sh, pu = range(0, N // 100), range(N - Z // 4 - 3 * N // 100, N - Z // 4)
        lin = C.RateMatch(N, sh, pu)
        Ncb = lin.E
        acc = torch.zeros((N, F), device="cuda")
        acc2 = torch.zeros((N, F), device="cuda")
        y = torch.empty((N, F), device="cuda")
        rx = torch.empty((2 * Ncb, F), device="cuda")
        tx = torch.empty((2 * Ncb, F), dtype=torch.int32, device="cuda")
        cw = torch.zeros((N, F), dtype=torch.int32, device="cuda")
        seed = np.array([173, 173, 173], np.int32)
        sp = seed.ctypes.data_as(ctypes.c_void_p)
        dones = {"none": torch.zeros(F, dtype=torch.int32, device="cuda"), "first half": torch.zeros(F, dtype=torch.int32, device="cuda"),
                 "every other": torch.zeros(F, dtype=torch.int32, device="cuda")}
        dones["first half"][:F // 2] = 1
        dones["every other"][1::2] = 1
        emit("# (a) %s N=%d Ncb=%d F=%d n_short=%d n_punct=%d" % (name, N, Ncb, F, lin.n_short, lin.n_punct))
        emit("# %-8s %-12s %24s %24s %8s" % ("E", "done", "fused ms", "select, channel, combine ms", "ratio"))
        fused_none = {}
        for laps in (1, 2):
            E = laps * Ncb
            rm = C.RateMatch.circular(N, sh, pu, Ncb // 3, E)
            fns = {}
            for dn, d in dones.items():
                def fused(d=d):
                    check(lib.bldpc_rm_awgn_combine_device(rm._h, sp, sigma, P(cw), F, llr, P(d), P(acc), st), "fused")

                def three(d=d):
                    check(lib.bldpc_rm_select(rm._h, P(cw), F, P(tx), st), "select")
                    check(lib.bldpc_awgn_channel_device(sp, sigma, P(rx), P(tx), E, F, st), "channel at E")
                    check(lib.bldpc_rm_combine(rm._h, P(rx), F, llr, P(d), P(acc2), st), "combine")

                fns["fused " + dn], fns["calls " + dn] = fused, three
            if laps == 1:  # (b): the linear profile's channel at the same number of samples
                fns["linear channel"] = lambda: check(lib.bldpc_rm_awgn_channel_device(lin._h, sp, sigma, P(cw), F, llr, P(y), st), "linear")
            for f in fns.values():
                for _ in range(2):
                    f()
            acc.zero_()
            acc2.zero_()
            torch.cuda.synchronize()
            t = timed_round(fns, args.reps)
            med = {k: float(np.median(v)) for k, v in t.items()}
            fmt = lambda k: "%8.3f [%6.3f .. %6.3f]" % (med[k], min(t[k]), max(t[k]))  # noqa: E731
            for dn in dones:
                emit("  %-8d %-12s %24s %24s %8.3f" % (E, dn, fmt("fused " + dn), fmt("calls " + dn), med["fused " + dn] / med["calls " + dn]))
            fused_none[laps] = med["fused none"]
            emit("  E=%d: fused, first half done / none = %.3f; every other done / none = %.3f" % (
                E, med["fused first half"] / med["fused none"], med["fused every other"] / med["fused none"]))
            if laps == 1:
                emit("# (b) %s E=Ncb=%d: fused channel + combine %s, bldpc_rm_awgn_channel_device on the linear profile %s, ratio %.3f" % (
                    name, E, fmt("fused none"), fmt("linear channel"), med["fused none"] / med["linear channel"]))
        emit("  fused, E = 2 Ncb / E = Ncb (no frame done) = %.3f" % (fused_none[2] / fused_none[1]))
        del acc, acc2, y, rx, tx, cw

    # (c) one sweep point, both settings of `compact` alternating; wall time of the whole call, counters read back included
    path = os.path.join(ROOT, "data", "bldpc", "J4_L24_Z96_BlockH.txt")
    code = C.BinaryCode.from_blockh(path, 4, 24, 96)
    rvs = [C.RateMatch.circular(code.N, range(0, 24), range(2188, 2260), k0, E) for k0, E in ((0, 2160), (2160, 48), (500, 2300))]
    F, batches, snr = 65536, 2, 2.7
    kw = dict(Num_Frames_OneTime=F, max_batches=batches, log=None, leastTestFrames=10 ** 12, PN_Message=1, pn_seed=1, alpha=0.75, maxIT=25,
              exit_mode=C.EXIT_PER_FRAME, schedule="layered")
    times = {True: [], False: []}
    SIM = None
    for rep in range(args.reps + 2):
        for compact in (True, False):
            SIM = HarqCounters()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            Simulation_HARQ_GPU(code, np.array([173, 173, 173], np.int32), C.sigma_of(snr), SIM, rvs, compact=compact, **kw)
            torch.cuda.synchronize()
            if rep >= 2:  # two warm-up rounds
                times[compact].append((time.perf_counter() - t0) * 1e3)
    n = SIM.num_Frames
    active = [1.0, (n - SIM.acked[0]) / n, (n - SIM.acked[0] - SIM.acked[1]) / n]
    emit("# (c) Simulation_HARQ_GPU, J4_L24_Z96, layered alpha 0.75, 25 iterations per-frame exit, random codewords, Es/N0 %.1f dB, "
         "%d batches of %d frames, transmissions (k0, E) = (0, 2160), (2160, 48), (500, 2300); wall ms of the call, %d repetitions" % (
             snr, batches, F, len(times[True])))
    emit("  acked %s undetected %s never %d; active fraction at the decodes %s, mean over the decodes run %.3f" % (
        SIM.acked, SIM.undetected, SIM.never_acked, ["%.3f" % a for a in active], sum(active) / len(active)))
    for compact in (True, False):
        v = times[compact]
        emit("  compact=%-5s %9.2f [%8.2f .. %8.2f]" % (compact, float(np.median(v)), min(v), max(v)))
    emit("  compact=True / compact=False = %.3f" % (float(np.median(times[True])) / float(np.median(times[False]))))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
