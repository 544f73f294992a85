"""What the fused receive calls of rate matching over GF(q) symbol vectors cost, one session on one card: each of
nbldpc_rm_demodulate_{qam,bpsk}_{recover,combine} against its composition, nbldpc_demodulate_*_nq at N := E followed by nbldpc_rm_recover
or nbldpc_rm_combine (no frame done, and the first half of the batch done), and both against one EMS(2,2) decode (20 iterations at most)
of the same batch's BPSK decoder input.  BDS.576.288.GF.64 (N = 96 symbols of GF(64)) with 16 384 frames and LDPC_N96_K48_GF256_d1_exp
(96 bits: N = 12 symbols of GF(256)) with 65 536; the last N / 12 symbols punctured; a linear profile, a one-lap circular profile
(k0 = Ncb / 3) and a three-lap one.
Whole calls of the C ABI between HIP events on the stream after warm-up, every output preallocated, the variants alternating inside
every repetition; median [min .. max].
usage: python tools/nb_rm_time.py [--reps R] [--out FILE]   (GPU box)"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cuda_ldpc_amd as C  # noqa: E402
from cuda_ldpc_amd import nbldpc as nb  # noqa: E402
from cuda_ldpc_amd._lib import lib  # noqa: E402
from harq_time import timed_round  # noqa: E402


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, lib.nbldpc_last_error().decode(errors="replace")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 7:
        ap.error("at least 7 repetitions")
    if not torch.cuda.is_available():
        sys.exit("nb_rm_time.py needs a GPU")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("# python tools/nb_rm_time.py --reps %d" % args.reps)
    emit("# %s, %d repetitions, C-ABI calls on preallocated outputs, alternating; ms = median [min .. max]; ratio = fused / calls; "
         "of decode = fused / one EMS(2,2) decode of the batch" % (torch.cuda.get_device_name(0), args.reps))
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    llr = ctypes.c_float(1.0e4)
    nbd = os.path.join(ROOT, "data", "nb")
    worst = {}
    for name, B in (("BDS.576.288.GF.64", 16384), ("LDPC_N96_K48_GF256_d1_exp", 65536)):
        H = nb.NBMatrix(os.path.join(nbd, name + ".txt"))
        q, m, N, V = H.q, H.m, H.N, H.q - 1
        mul, _, _ = nb.GFInitial(q, os.path.join(nbd, "GF", "Arith.Table.GF.%d.txt" % q))
        code = nb.NBCode(os.path.join(nbd, name + ".txt"), mul)
        con = torch.from_numpy(nb.Get_CONSTELLATION(os.path.join(nbd, "Constellation", "GRAY_%dQAM.txt" % q), q)).cuda()
        pu = range(N - N // 12, N)
        Ncb = N - len(pu)
        g = torch.Generator(device="cuda").manual_seed(N + q)
        out, out2 = torch.zeros((B, N, V), device="cuda"), torch.zeros((B, N, V), device="cuda")
        tmp = torch.empty((B, 3 * Ncb, V), device="cuda")
        dones = {"none": torch.zeros(B, dtype=torch.int32, device="cuda"), "first half": torch.zeros(B, dtype=torch.int32, device="cuda")}
        dones["first half"][:B // 2] = 1
        dec = [torch.empty((B, N), dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda"),
               torch.empty(B, dtype=torch.int32, device="cuda")]
        emit("# %s N=%d q=%d B=%d n_punct=%d Ncb=%d; output %.0f MB" % (name, N, q, B, len(pu), Ncb, B * N * V * 4 / 1e6))
        emit("# %-11s %-5s %-5s %-24s %24s %24s %7s %10s" % ("profile", "E", "chain", "call", "fused ms", "calls ms", "ratio", "of decode"))
        for pname, rm in (("linear", C.RateMatch(N, (), pu)), ("circ 1 lap", C.RateMatch.circular(N, (), pu, Ncb // 3, Ncb)),
                          ("circ 3 laps", C.RateMatch.circular(N, (), pu, Ncb // 3, 3 * Ncb))):
            E = rm.E
            sym = nb.RM_Select(rm, nb.PN_CodeWords(code, 1, B)).long()  # the transmitted symbols of B random codewords
            sq, sb = ctypes.c_float(0.1), ctypes.c_float(0.6)
            rxq = (con[sym] + 0.1 * torch.randn((B, E, 2), generator=g, device="cuda")).contiguous()
            bits = ((sym[:, :, None] >> torch.arange(m, device="cuda")) & 1).to(torch.float32)
            rxb = ((1.0 - 2.0 * bits) + 0.6 * torch.randn((B, E, m), generator=g, device="cuda")).reshape(B, E * m).contiguous()
            fns = {}

            def add(chain, rx, sig, fused_rec, fused_com, demod):
                def frec():
                    check(fused_rec(rx, sig, out), "fused recover")

                def crec():
                    check(demod(rx, sig), "demodulate")
                    check(lib.nbldpc_rm_recover(rm._h, q, P(tmp), B, llr, P(out2), st), "recover")

                fns[chain, "fused", "recover"], fns[chain, "calls", "recover"] = frec, crec
                for dn, d in dones.items():
                    def fcom(d=d):
                        check(fused_com(rx, sig, d, out), "fused combine")

                    def ccom(d=d):
                        check(demod(rx, sig), "demodulate")
                        check(lib.nbldpc_rm_combine(rm._h, q, P(tmp), B, llr, P(d), P(out2), st), "combine")

                    fns[chain, "fused", "combine, done " + dn], fns[chain, "calls", "combine, done " + dn] = fcom, ccom

            add("qam", rxq, sq, lambda rx, s, o: lib.nbldpc_rm_demodulate_qam_recover(rm._h, q, P(rx), P(con), s, B, llr, P(o), st),
                lambda rx, s, d, o: lib.nbldpc_rm_demodulate_qam_combine(rm._h, q, P(rx), P(con), s, B, llr, P(d), P(o), st),
                lambda rx, s: lib.nbldpc_demodulate_qam_nq(E, q, P(rx), P(con), s, B, P(tmp), st))
            add("bpsk", rxb, sb, lambda rx, s, o: lib.nbldpc_rm_demodulate_bpsk_recover(rm._h, q, P(rx), s, B, llr, P(o), st),
                lambda rx, s, d, o: lib.nbldpc_rm_demodulate_bpsk_combine(rm._h, q, P(rx), s, B, llr, P(d), P(o), st),
                lambda rx, s: lib.nbldpc_demodulate_bpsk_nq(E, q, P(rx), s, B, P(tmp), st))
            Lch = nb.RM_Demodulate_Recover(rm, q, rxb, 0.6)  # the decoder input of this batch over BPSK

            def decode():
                check(lib.nbldpc_ems_decode_batch(code._h, P(Lch), B, 2, 2, 20, 0, P(dec[0]), P(dec[1]), P(dec[2]), None, None, st), "decode")

            fns["-", "decode", "-"] = decode
            for f in fns.values():
                for _ in range(2):
                    f()
            torch.cuda.synchronize()
            t = timed_round(fns, args.reps)
            med = {k: float(np.median(v)) for k, v in t.items()}
            fmt = lambda k: "%8.3f [%6.3f .. %6.3f]" % (med[k], min(t[k]), max(t[k]))  # noqa: E731
            for chain in ("qam", "bpsk"):
                for call in ("recover", "combine, done none", "combine, done first half"):
                    r = med[chain, "fused", call] / med[chain, "calls", call]
                    emit("  %-11s %-5d %-5s %-24s %24s %24s %7.3f %10.4f" % (pname, E, chain, call, fmt((chain, "fused", call)), fmt((chain, "calls", call)),
                                                                           r, med[chain, "fused", call] / med["-", "decode", "-"]))
                    worst[chain, call.split(",")[0]] = max(worst.get((chain, call.split(",")[0]), 0.0), r)
            emit("  %-11s %-5d %-5s %-24s %24s   (ok %d of %d)" % (pname, E, "bpsk", "EMS(2,2) decode", fmt(("-", "decode", "-")), int(dec[2].sum()), B))
            out.zero_()
            out2.zero_()
            del sym, rxq, rxb, bits, Lch
        del out, out2, tmp
    for (chain, call), r in sorted(worst.items()):
        emit("# the largest ratio fused / calls of %s %s over the cases: %.3f" % (chain, call, r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
