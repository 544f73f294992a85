"""What the fused calls of rate matching over QAM cost, one session on one card:
  (a) bldpc_rm_qam_map against the two calls it replaces, bldpc_rm_select and bldpc_qam_map_il at N := E;
  (b) bldpc_rm_qam_recover against bldpc_qam_demap_il at N := E and bldpc_rm_recover, and bldpc_rm_qam_combine against
      bldpc_qam_demap_il and bldpc_rm_combine with no frame done and with the first half of the batch done;
  (c) one HARQ sweep point, Simulation_HARQ_GPU on J4_L24_Z96 over 64-QAM with the row-column interleaver next to the BPSK point of
      tools/harq_time.py (c), same profiles, decoder and frame counts, each at an operating point inside its own waterfall.
(a) and (b) on J4_L24_Z96 with 65 536 frames and PON_LDPC (J12_L69_Z256) with 4 096, about 1 % of the positions shortened and 3 %
punctured as in tools/harq_time.py; 64- and 256-QAM; both index rules; E = Ncb (one lap, one launch of the demapper) and E = 2 Ncb (two
laps, two launches: under the row-column rule each walks every symbol).  Whole calls of the C ABI between HIP events on the stream
after warm-up, every output preallocated, the variants alternating inside every repetition; median [min .. max].
usage: python tools/harq_qam_time.py [--reps R] [--out FILE]   (GPU box)"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cuda_ldpc_amd as C  # noqa: E402
from cuda_ldpc_amd import nbldpc as nb  # noqa: E402
from cuda_ldpc_amd._lib import check, lib  # noqa: E402
from cuda_ldpc_amd.simulation import HarqCounters, Simulation_HARQ_GPU  # noqa: E402
from harq_time import timed_round  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("at least 7 repetitions")
    if not torch.cuda.is_available():
        sys.exit("harq_qam_time.py needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# python tools/harq_qam_time.py --reps %d" % args.reps)
    emit("# %s, %d repetitions, C-ABI calls on preallocated outputs, alternating; ms = median [min .. max]; ratio = fused / calls" % (
        torch.cuda.get_device_name(0), args.reps))
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    llr, scale = ctypes.c_float(1.0e4), ctypes.c_float(1.0 / (2 * 0.1 * 0.1))
    cons = {q: torch.from_numpy(C.Get_CONSTELLATION(os.path.join(ROOT, "data", "nb", "Constellation", "GRAY_%dQAM.txt" % q), q)).cuda()
            for q in (64, 256)}
    worst = {}  # laps -> the largest ratio of medians of a fused receive call
    for name, L, Z, F in (("J4_L24_Z96", 24, 96, 65536), ("PON_LDPC", 69, 256, 4096)):
        N = L * Z
        sh, pu = range(0, N // 100), range(N - Z // 4 - 3 * N // 100, N - Z // 4)
        Ncb = N - len(sh) - len(pu)
        g = torch.Generator(device="cuda").manual_seed(N)
        cw = torch.randint(0, 2, (N, F), generator=g, device="cuda", dtype=torch.int32)
        tx = torch.empty((2 * Ncb, F), dtype=torch.int32, device="cuda")
        tmp = torch.empty((2 * Ncb, F), device="cuda")
        out, out2 = torch.zeros((N, F), device="cuda"), torch.zeros((N, F), device="cuda")
        dones = {"none": torch.zeros(F, dtype=torch.int32, device="cuda"), "first half": torch.zeros(F, dtype=torch.int32, device="cuda")}
        dones["first half"][:F // 2] = 1
        emit("# %s N=%d Ncb=%d F=%d n_short=%d n_punct=%d" % (name, N, Ncb, F, len(sh), len(pu)))
        emit("# %-4s %-7s %-8s %-22s %24s %24s %8s" % ("q", "rule", "E", "call", "fused ms", "calls ms", "ratio"))
        for q, con in cons.items():
            m = q.bit_length() - 1
            for il, rule in ((C.IL_NONE, "none"), (C.IL_ROWCOL, "rowcol")):
                for laps in (1, 2):
                    E = laps * Ncb
                    rm = C.RateMatch.circular(N, sh, pu, Ncb // 3, E)
                    Ns = (E + m - 1) // m
                    sym, sym2 = (torch.empty((F, Ns), dtype=torch.int32, device="cuda") for _ in range(2))
                    rx = (con[torch.randint(0, q, (F, Ns), generator=g, device="cuda")] + 0.1 * torch.randn((F, Ns, 2), generator=g, device="cuda")).contiguous()
                    fns = {}

                    def fmap():
                        check(lib.bldpc_rm_qam_map(rm._h, P(cw), F, m, il, P(sym), st), "rm_qam_map")

                    def cmap():
                        check(lib.bldpc_rm_select(rm._h, P(cw), F, P(tx), st), "select")
                        check(lib.bldpc_qam_map_il(P(tx), E, F, m, il, P(sym2), st), "map")

                    def frec():
                        check(lib.bldpc_rm_qam_recover(rm._h, P(rx), P(con), q, scale, il, F, llr, P(out), st), "rm_qam_recover")

                    def crec():
                        check(lib.bldpc_qam_demap_il(P(rx), P(con), q, scale, E, F, il, P(tmp), st), "demap")
                        check(lib.bldpc_rm_recover(rm._h, P(tmp), F, llr, P(out2), st), "recover")

                    fns["fused map"], fns["calls map"], fns["fused recover"], fns["calls recover"] = fmap, cmap, frec, crec
                    for dn, d in dones.items():
                        def fcom(d=d):
                            check(lib.bldpc_rm_qam_combine(rm._h, P(rx), P(con), q, scale, il, F, llr, P(d), P(out), st), "rm_qam_combine")

                        def ccom(d=d):
                            check(lib.bldpc_qam_demap_il(P(rx), P(con), q, scale, E, F, il, P(tmp), st), "demap")
                            check(lib.bldpc_rm_combine(rm._h, P(tmp), F, llr, P(d), P(out2), st), "combine")

                        fns["fused combine, done " + dn], fns["calls combine, done " + dn] = fcom, ccom
                    for f in fns.values():
                        for _ in range(2):
                            f()
                    torch.cuda.synchronize()
                    assert torch.equal(sym, sym2)
                    t = timed_round(fns, args.reps)
                    med = {k: float(np.median(v)) for k, v in t.items()}
                    fmt = lambda k: "%8.3f [%6.3f .. %6.3f]" % (med[k], min(t[k]), max(t[k]))  # noqa: E731
                    for call in ("map", "recover", "combine, done none", "combine, done first half"):
                        r = med["fused " + call] / med["calls " + call]
                        emit("  %-4d %-7s %-8d %-22s %24s %24s %8.3f" % (q, rule, E, call, fmt("fused " + call), fmt("calls " + call), r))
                        if call != "map":
                            worst[laps, rule] = max(worst.get((laps, rule), 0.0), r)
                    out.zero_()
                    out2.zero_()
                    del sym, sym2, rx
        del cw, tx, tmp, out, out2
    for (laps, rule), r in sorted(worst.items()):
        emit("# the largest ratio of a fused receive call (recover, combine) at %d lap(s), rule %s: %.3f" % (laps, rule, r))

    # (c) one sweep point over 64-QAM next to the BPSK point of harq_time.py (c); wall time of the whole call, counters read back included
    path = os.path.join(ROOT, "data", "bldpc", "J4_L24_Z96_BlockH.txt")
    code = C.BinaryCode.from_blockh(path, 4, 24, 96)
    rvs = [C.RateMatch.circular(code.N, range(0, 24), range(2188, 2260), k0, E) for k0, E in ((0, 2160), (2160, 48), (500, 2300))]
    F, batches = 65536, 2
    kw = dict(Num_Frames_OneTime=F, max_batches=batches, log=None, leastTestFrames=10 ** 12, PN_Message=1, pn_seed=1, alpha=0.75, maxIT=25,
              exit_mode=C.EXIT_PER_FRAME, schedule="layered")
    con64 = cons[64].cpu().numpy()
    points = {"BPSK, Es/N0 2.7 dB": (C.sigma_of(2.7), {}),
              "64-QAM rowcol, Eb/N0 11.0 dB": (nb.sigma_of(11.0, rvs[0].rate(code.K), 0, 64), dict(n_QAM=64, CONSTELLATION=con64, interleave=C.IL_ROWCOL))}
    times, sims = {k: [] for k in points}, {}
    for rep in range(args.reps + 2):
        for k, (sigma, mod) in points.items():
            SIM = HarqCounters()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            Simulation_HARQ_GPU(code, np.array([173, 173, 173], np.int32), sigma, SIM, rvs, **kw, **mod)
            torch.cuda.synchronize()
            if rep >= 2:  # two warm-up rounds
                times[k].append((time.perf_counter() - t0) * 1e3)
            sims[k] = SIM
    emit("# (c) Simulation_HARQ_GPU, J4_L24_Z96, layered alpha 0.75, 25 iterations per-frame exit, random codewords, compact=True, %d batches of "
         "%d frames, transmissions (k0, E) = (0, 2160), (2160, 48), (500, 2300); wall ms of the call, %d repetitions" % (batches, F, args.reps))
    for k, v in times.items():
        S = sims[k]
        emit("  %-30s %9.2f [%8.2f .. %8.2f]   acked %s undetected %s never %d" % (k, float(np.median(v)), min(v), max(v), S.acked, S.undetected,
                                                                                S.never_acked))
    ks = list(points)
    emit("  64-QAM / BPSK = %.3f" % (float(np.median(times[ks[1]])) / float(np.median(times[ks[0]]))))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
