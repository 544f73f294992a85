#!/usr/bin/env python3
"""BER/FER sweeps in the reference's output format, driven through the C ABI.

    python sweep.py binary --matrix data/bldpc/J4_L24_Z96_BlockH.txt --J 4 --L 24 --Z 96 --start 0 --stop 4.4 --step 0.2
    python sweep.py nb     --start 0 --stop 5 --step 0.5
    python sweep.py binary --device-channel --layered --per-frame --pn-message --harq 0:2160,2160:144,500:2400 --start 2 --stop 3 --step 0.5
    python sweep.py binary --device-channel --layered --per-frame --pn-message --qam 64 --interleave rowcol --snrtype 0 --harq 0:2160,2160:144,500:2400 --start 8 --stop 9 --step 0.5
    python sweep.py binary --device-channel --bp --per-frame --stop-rule syndrome --pn-message --start 2 --stop 3 --step 0.2
    python sweep.py binary --device-channel --quant 6,8,6 --norm8 6 --llr-scale 16 --per-frame --stop-rule syndrome --pn-message --start 2 --stop 3 --step 0.2
    python sweep.py binary --hard gradient --per-frame --pn-message --bsc 0.002,0.004,0.006
    python sweep.py binary --hard threshold --device-channel --per-frame --start 4 --stop 6 --step 0.5
    python sweep.py binary --erasure --bec 0.08,0.10,0.12,0.14 --pn-message --puncture 2208:2304 --iters 100
    python sweep.py binary --erasure --bec 0.12,0.14,0.16 --ml
    python sweep.py binary --device-channel --per-frame --layered --alpha 0.75 --stop-rule syndrome --osd
    python sweep.py binary --device-channel --per-frame --layered --pn-message --qam 64 --interleave rowcol --fading 16 --harq 0:2160,2160:48,500:2300
    python sweep.py nb --pn-message --qam 64 --fading 16
    python sweep.py nb --device-channel --pn-message --puncture 88:96
    python sweep.py nb --device-channel --pn-message --harq 0:72,72:48,24:96
    python -m torch.distributed.run --nproc-per-node N sweep.py binary ...      (frames sharded over N GPUs)

binary: rows `SNR NTF NEF FER BER AverIT FER_F FER_A` as Simulation.cu:272 prints them (Es/N0, seeds 173/173/173,
batches of --batch frames, stop at >= 50 error frames and >= 10000 frames, or --max-batches).
        with --harq: rows `SNR NTF FER-after-each-transmission mean-transmissions throughput AverIT` (Simulation_HARQ_GPU).
nb:     rows `SNR NTF NEF FER BER AverIT` as Simulation.cpp:198 (Eb/N0, stop at >= 50 error frames and >= 1000 frames).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def parse_positions(spec, N=None):
    """SPEC of --shorten / --puncture: comma-separated half-open ranges a:b of codeword positions -> sorted list of positions."""
    pos = set()
    for part in spec.split(","):
        a, sep, b = part.strip().partition(":")
        if not sep or not a.strip().isdigit() or not b.strip().isdigit() or int(a) >= int(b):
            raise ValueError("%r is not a range a:b of codeword positions with a < b" % part)
        if N is not None and int(b) > N:
            raise ValueError("range %s ends past N=%d" % (part.strip(), N))
        pos.update(range(int(a), int(b)))
    return sorted(pos)


def parse_harq(spec):
    """SPEC of --harq: comma-separated K0:E, one per transmission -> [(k0, E), ...]."""
    out = []
    for part in spec.split(","):
        a, sep, b = part.strip().partition(":")
        if not sep or not a.strip().isdigit() or not b.strip().isdigit() or int(b) < 1:
            raise ValueError("%r is not K0:E with a buffer start K0 >= 0 and a length E >= 1" % part)
        out.append((int(a), int(b)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("which", choices=["binary", "nb"])
    ap.add_argument("--matrix", default=os.path.join(ROOT, "data", "bldpc", "J4_L24_Z96_BlockH.txt"))
    ap.add_argument("--J", type=int, default=4)
    ap.add_argument("--L", type=int, default=24)
    ap.add_argument("--Z", type=int, default=96)
    ap.add_argument("--start", type=float, default=0.0)
    ap.add_argument("--stop", type=float, default=4.4)
    ap.add_argument("--step", type=float, default=0.2)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--max-batches", type=int, default=None)
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--fixed", action="store_true", help="fixed iteration count instead of the reference's batch-global early exit")
    ap.add_argument("--per-frame", action="store_true", help="binary: every frame stops on its own flag (the reference rule with Num_Frames_OneTime = 1)")
    ap.add_argument("--qam", type=int, default=2, choices=[2, 64, 256],
                    help="n_QAM (define.h:25): 2 = BPSK, q = Constellation/GRAY_<q>QAM.txt; nb: one point per GF(q) symbol; binary: log2 q "
                         "codeword bits per point, max-log demapper, Eb/N0 as in the nb sweep (needs --pn-message --device-channel)")
    ap.add_argument("--interleave", choices=["none", "rowcol"], default="none", help="binary --qam: the bit interleaver between the codeword (or "
                    "the rate-matched bits) and the points: none = consecutive bits share a point, rowcol = the row-column interleaver")
    ap.add_argument("--nb-matrix", default="BDS.576.288.GF.64.txt", help="nb: matrix file (under data/nb or a path); q from its header")
    ap.add_argument("--method", type=int, default=0, choices=[0, 1, 2, 3, 4, 5],
                    help="NB decoder_method (define.h:37): 0 EMS, 1 TMM, 2 log-QSPA, 3 layered TMM; ours: 4 FHT sum-product, 5 layered FHT sum-product")
    ap.add_argument("--qspa-tier", default="lds", choices=["lds", "workspace", "auto"],
                    help="NB --method 4|5: the tier of the FHT sum-product decoder; lds keeps a frame in LDS and refuses a code over its bound, "
                         "workspace keeps it in a global-memory workspace, auto takes the workspace where lds refuses")
    ap.add_argument("--device-channel", action="store_true", help="generate the AWGN samples on the GPU (same RNG draws, device libm)")
    ap.add_argument("--pn-message", action="store_true", help="send random codewords (PN_Message 1, define.cuh:26); binary: needs --fixed")
    ap.add_argument("--pn-seed", type=int, default=1, help="--pn-message: seed of the message stream (bldpc_encode_random / nbldpc_encode_random)")
    ap.add_argument("--layered", action="store_true", help="binary: row-layered normalised min-sum (bldpc_decode_layered); with --fixed or --per-frame")
    ap.add_argument("--bp", action="store_true", help="binary: row-layered sum-product (bldpc_decode_layered_bp, llr_scale = 2 / sigma^2 over BPSK, "
                    "1 over QAM); with --fixed or --per-frame, takes --stop-rule and every channel option, no --alpha")
    ap.add_argument("--quant", metavar="CH,APP,MSG", default=None, help="binary: row-layered min-sum with finite word lengths "
                    "(bldpc_decode_layered_quant): bits of the channel, a-posteriori and check-message words; with --fixed or --per-frame, takes "
                    "--stop-rule and every channel option, no --alpha")
    ap.add_argument("--norm8", type=int, default=6, help="--quant: normalisation in eighths, rounded (8 = none)")
    ap.add_argument("--quant-offset", type=int, default=0, help="--quant: offset subtracted after the normalisation")
    ap.add_argument("--llr-scale", type=float, default=16.0, help="--quant: quantiser gain on the channel value (resolution only: min-sum is "
                    "scale-invariant; below about 16 the rate-5/6 codes lose error rate)")
    ap.add_argument("--hard", choices=["threshold", "gradient"], default=None, help="binary: hard-decision decoding by parallel bit flipping "
                    "(bldpc_decode_bitflip) on the hard decisions of the channel values: threshold = flip iff 2 u + e > d, gradient = flip the "
                    "variables of largest u + e; with --device-channel and --fixed or --per-frame; no --alpha, --stop-rule, --shorten / --puncture, --harq")
    ap.add_argument("--bsc", metavar="P[,P...]", default=None, help="--hard: crossover probabilities of a binary symmetric channel in place of the "
                    "SNR list (Simulation_BSC_GPU; the first column of a row is P)")
    ap.add_argument("--erasure", action="store_true", help="binary: erasure decoding by parallel peeling (bldpc_decode_erasure) on packed words over "
                    "a binary erasure channel, with --bec; takes --pn-message, --shorten / --puncture (punctured = erased, shortened = known 0) and "
                    "--iters; no --hard, --layered, --bp, --quant, --qam, --fading, --harq")
    ap.add_argument("--bec", metavar="P[,P...]", default=None, help="--erasure: erasure probabilities of the binary erasure channel in place of the "
                    "SNR list (Simulation_BEC_GPU; the first column of a row is P)")
    ap.add_argument("--ml", action="store_true", help="--erasure: after peeling, maximum-likelihood decoding by elimination over GF(2) on the frames "
                    "peeling leaves stuck (bldpc_decode_erasure_ml)")
    ap.add_argument("--ml-max-erased", type=int, default=0, metavar="E", help="--ml: frames with more than E positions still erased are left as "
                    "peeling left them (default 0: the number of check rows)")
    ap.add_argument("--osd", action="store_true", help="binary --layered / --bp / --quant with the syndrome stop rule: ordered-statistics "
                    "reprocessing of order 0 (bldpc_decode_osd) on the frames the decoder leaves with a non-zero syndrome; the row ends with the "
                    "frames reprocessed and those of them that came out equal to the word sent")
    ap.add_argument("--osd-order", type=int, choices=(0, 1, 2), default=0, help="--osd: also every single trusted position flipped (1) and the pairs "
                    "among the --osd-lambda least reliable of them (2), the candidate of least soft metric kept (bldpc_decode_osd_w)")
    ap.add_argument("--osd-lambda", type=int, default=0, metavar="L", help="--osd --osd-order 2: pairs among the first L positions outside the basis")
    ap.add_argument("--alpha", type=float, default=1.0, help="binary: normalisation factor in (0, 1]; with --layered the layered decoder's, without it "
                    "normalised min-sum on the flooding decoders (with --fixed or --per-frame)")
    ap.add_argument("--stop-rule", choices=["prefix", "syndrome"], default=None,
                    help="--layered / --bp: stop rule / meaning of the flag row (default: syndrome with --pn-message, else prefix)")
    ap.add_argument("--as-written", action="store_true", help="decode on the reference's Transform_H table as written (SURVEY F3)")
    ap.add_argument("--shorten", metavar="SPEC", default=None, help="codeword positions (binary: bits, nb: symbols) fixed to 0 and not sent, "
                    "comma-separated half-open ranges a:b (information positions; needs --device-channel)")
    ap.add_argument("--puncture", metavar="SPEC", default=None, help="codeword positions (binary: bits, nb: symbols) not sent, same SPEC (needs --device-channel)")
    ap.add_argument("--short-llr", type=float, default=1.0e4, help="--shorten: the decoder's input on a shortened position")
    ap.add_argument("--harq", metavar="K0:E[,K0:E...]", default=None, help="incremental-redundancy HARQ over BPSK or --qam (nb: symbol-LLR combining, K0 and E in symbols, Eb/N0 by default), one circular-buffer "
                    "transmission per K0:E (start in the buffer of the positions left by --shorten / --puncture, length; E above the buffer "
                    "repeats); only unacknowledged frames are sent and decoded again; --snrtype applies, sigma under Eb/N0 from the FIRST "
                    "transmission's rate (needs --device-channel and --fixed or --per-frame)")
    ap.add_argument("--snrtype", type=int, default=None, choices=[0, 1], help="--harq: 0 = Eb/N0 on the first transmission's rate, 1 = Es/N0 (default)")
    ap.add_argument("--no-compact", action="store_true", help="--harq: decode the whole batch after every transmission (timing and checking)")
    ap.add_argument("--fading", metavar="LC", type=int, default=None, help="flat Rayleigh block fading with receiver CSI: gains constant over LC "
                    "channel uses (bits over BPSK, points over QAM), 1 = fast fading, 0 = quasi-static (one gain per frame and transmission); "
                    "binary: needs --device-channel and --fixed or --per-frame, combines with --qam, --interleave, --shorten / --puncture, "
                    "--harq and every decoder; nb: needs --qam 64/256 and runs on the device channel")
    ap.add_argument("--fade-seed", metavar="A,B,C", default=None, help="--fading: the seed of the fading stream (default 4711,4712,4713)")
    args = ap.parse_args()
    fade = None
    if args.fading is not None:
        try:
            fade_seed = tuple(int(x) for x in (args.fade_seed or "4711,4712,4713").split(","))
        except ValueError:
            ap.error("--fade-seed takes three integers A,B,C")
        if args.fading < 0 or len(fade_seed) != 3:
            ap.error("--fading takes LC >= 0 and --fade-seed three integers A,B,C")
        if args.which == "binary" and (not args.device_channel or not (args.fixed or args.per_frame) or args.as_written):
            ap.error("binary --fading needs --device-channel and --fixed or --per-frame (the batch-global exit depends on the batch)")
        if args.which == "nb" and args.qam == 2:
            ap.error("nb --fading needs --qam 64 or 256: the GF(q) BPSK path has no fading channel")
        fade = (args.fading, fade_seed)  # becomes a Fading once the package is imported
    elif args.fade_seed is not None:
        ap.error("--fade-seed belongs to --fading")
    if args.harq is not None:
        if not args.device_channel or (args.which == "binary" and (args.as_written or not (args.fixed or args.per_frame))):
            ap.error("--harq needs --device-channel and, in the binary sweep, --fixed or --per-frame")
        try:
            harq = parse_harq(args.harq)
        except ValueError as e:
            ap.error(str(e))
    elif args.snrtype is not None or args.no_compact:
        ap.error("--snrtype and --no-compact belong to --harq")
    if args.interleave != "none" and (args.which != "binary" or args.qam == 2):
        ap.error("--interleave belongs to the binary sweep with --qam")
    if args.bp and (args.which != "binary" or args.layered or args.alpha != 1.0):
        ap.error("--bp belongs to the binary sweep, without --layered and without --alpha (sum-product has no normalisation factor)")
    quant = None
    if args.quant is not None:
        if args.which != "binary" or args.layered or args.bp or args.alpha != 1.0:
            ap.error("--quant belongs to the binary sweep, without --layered, --bp and --alpha (--norm8 and --quant-offset are its correction)")
        try:
            ch, app, msg = (int(x) for x in args.quant.split(","))
        except ValueError:
            ap.error("--quant takes three integers CH,APP,MSG")
        quant = (ch, app, msg, args.norm8, args.quant_offset, args.llr_scale)  # checked by Quant once the package is imported
    elif args.norm8 != 6 or args.quant_offset != 0 or args.llr_scale != 16.0:
        ap.error("--norm8, --quant-offset and --llr-scale belong to --quant")
    bsc = None
    if args.hard is not None:
        if (args.which != "binary" or args.layered or args.bp or quant is not None or args.alpha != 1.0 or args.stop_rule is not None or args.as_written
                or args.shorten is not None or args.puncture is not None or args.harq is not None or not (args.fixed or args.per_frame)):
            ap.error("--hard belongs to the binary sweep on a QC code with --fixed or --per-frame, without --layered, --bp, --quant, --alpha, "
                     "--stop-rule, --shorten, --puncture and --harq (a hard decoder has no value for an unsent position)")
        if args.bsc is not None:
            try:
                bsc = [float(x) for x in args.bsc.split(",")]
            except ValueError:
                ap.error("--bsc takes crossover probabilities P[,P...]")
            if not bsc or not all(0.0 <= x <= 0.5 for x in bsc) or args.qam != 2 or fade is not None:
                ap.error("--bsc takes probabilities in [0, 0.5] and replaces the channel: no --qam, no --fading")
        elif not args.device_channel:
            ap.error("--hard without --bsc needs --device-channel")
    elif args.bsc is not None:
        ap.error("--bsc belongs to --hard")
    bec = None
    if args.erasure:
        if (args.which != "binary" or args.hard is not None or args.layered or args.bp or quant is not None or args.qam != 2 or fade is not None
                or args.harq is not None or args.alpha != 1.0 or args.stop_rule is not None or args.as_written or args.fixed or args.per_frame):
            ap.error("--erasure belongs to the binary sweep on a QC code, without --hard, --layered, --bp, --quant, --qam, --fading, --harq, --alpha "
                     "and --stop-rule; peeling has no exit mode, so no --fixed / --per-frame either")
        try:
            bec = [float(x) for x in (args.bec or "").split(",")]
        except ValueError:
            ap.error("--erasure needs --bec P[,P...], erasure probabilities")
        if not all(0.0 <= x <= 1.0 for x in bec):
            ap.error("--bec takes probabilities in [0, 1]")
    elif args.bec is not None:
        ap.error("--bec belongs to --erasure")
    if (args.ml or args.ml_max_erased) and not args.erasure:
        ap.error("--ml and --ml-max-erased belong to --erasure")
    if args.ml_max_erased and not args.ml:
        ap.error("--ml-max-erased belongs to --ml")
    if args.ml_max_erased < 0:
        ap.error("--ml-max-erased takes a count of erased positions, 0 for the number of check rows")
    rows = args.layered or args.bp or quant is not None  # the row-layered decoders take the same modes and rules
    if args.which == "binary" and rows:
        if args.as_written or not (args.fixed or args.per_frame):
            ap.error("--layered / --bp / --quant need a QC code and --fixed or --per-frame")
        if args.pn_message and args.per_frame and args.stop_rule == "prefix":
            ap.error("--pn-message --per-frame needs --stop-rule syndrome (the prefix rule tests for the all-zero word)")
        if args.osd and (args.stop_rule or ("syndrome" if args.pn_message else "prefix")) != "syndrome":
            ap.error("--osd needs --stop-rule syndrome (the frames to reprocess are those whose flag says 'no codeword')")
    elif args.osd:
        ap.error("--osd belongs to the binary sweep with --layered, --bp or --quant")
    elif args.stop_rule is not None or (args.alpha != 1.0 and args.which != "binary"):
        ap.error("--stop-rule belongs to the binary sweep with --layered, --bp or --quant, --alpha to the binary sweep")
    if (args.osd_order or args.osd_lambda) and not args.osd:
        ap.error("--osd-order and --osd-lambda belong to --osd")
    if args.osd_lambda < 0:
        ap.error("--osd-lambda must not be negative")
    elif args.alpha != 1.0 and not (args.fixed or args.per_frame):
        ap.error("--alpha without --layered (normalised flooding min-sum) needs --fixed or --per-frame")
    if args.which == "binary" and not rows and args.hard is None and not args.erasure and args.pn_message and (not args.fixed or args.as_written):
        ap.error("--pn-message needs the binary sweep with --fixed (the decoders' early exit tests for the all-zero word) on a QC code")
    if args.which == "binary" and args.qam != 2 and not (args.pn_message and args.device_channel):
        ap.error("binary --qam %d needs --pn-message (a QAM channel is not symmetric: the all-zero word is not representative) and "
                 "--device-channel (there is no host QAM channel on this path)" % args.qam)
    ratematch = args.shorten is not None or args.puncture is not None or args.harq is not None
    if ratematch:
        if not args.device_channel and not args.erasure:
            ap.error("--shorten / --puncture / --harq need --device-channel")
        try:  # binary: bit positions; nb: symbol positions, checked against N once the matrix header is read
            rm_N = args.L * args.Z if args.which == "binary" else None
            shorten = parse_positions(args.shorten, rm_N) if args.shorten else []
            puncture = parse_positions(args.puncture, rm_N) if args.puncture else []
        except ValueError as e:
            ap.error(str(e))
        if not (args.short_llr > 0 and args.short_llr < float("inf")):
            ap.error("--short-llr must be finite and > 0")
    nbd = os.path.join(ROOT, "data", "nb")
    if args.which == "nb":
        mpath = args.nb_matrix if os.path.exists(args.nb_matrix) else os.path.join(nbd, args.nb_matrix)
        with open(mpath) as f:
            nb_N, _, nb_q = (int(x) for x in f.readline().split()[:3])  # header "N M q" (Get_H, Simulation.cpp:355)
        if ratematch and max(shorten + puncture + [0]) >= nb_N:
            ap.error("--shorten / --puncture: a position past N=%d symbols" % nb_N)
        if ratematch and (args.qam != 2 or fade is not None):
            ap.error("nb --shorten / --puncture / --harq run over BPSK: the GF(q) simulations have no rate-matched QAM or fading chain "
                     "(DESIGN.md 4.19)")
        if not os.path.exists(os.path.join(nbd, "GF", "Arith.Table.GF.%d.txt" % nb_q)):
            ap.error("no GF/Arith.Table.GF.%d.txt for the field of %s" % (nb_q, args.nb_matrix))
        if args.qam != 2 and args.qam != nb_q:
            ap.error("--qam %d needs a GF(%d) code (one constellation point per symbol); %s is over GF(%d)" % (args.qam, args.qam, args.nb_matrix, nb_q))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    rank = int(os.environ.get("RANK", "0"))
    import cuda_ldpc_amd as C
    fad = {}
    if fade is not None:
        fad = dict(fading=C.Fading(fade[0] or C.QUASI_STATIC, fade[1]))
        try:
            fad["fading"].check()
        except ValueError as e:
            ap.error("--fade-seed: %s" % e)
        fade_words = ", Rayleigh block fading %s (seed %s), receiver CSI" % (
            "Lc=%d" % fade[0] if fade[0] else "quasi-static", ",".join(str(x) for x in fade[1]))

    if args.which == "binary":
        from cuda_ldpc_amd.simulation import sweep
        if args.as_written:
            H, wc, wv = C.Get_H(args.matrix, args.J, args.L)
            code = C.BinaryCode.from_table(args.J, args.L, args.Z, wc, wv, C.Transform_H(H, args.J, args.L, args.Z, wc, wv, as_written=True))
        else:
            code = C.BinaryCode.from_blockh(args.matrix, args.J, args.L, args.Z)
        lay = {}
        if not args.layered and args.alpha != 1.0:
            lay = dict(alpha=args.alpha)
        if rows:
            stop = args.stop_rule or ("syndrome" if args.pn_message else "prefix")
            lay = dict(schedule="layered", alpha=args.alpha, stop_rule=C.STOP_SYNDROME if stop == "syndrome" else C.STOP_PREFIX)
            if args.bp:
                lay = dict(schedule="bp", stop_rule=lay["stop_rule"])
            if quant is not None:
                try:
                    lay = dict(schedule="quant", quant=C.Quant(*quant), stop_rule=lay["stop_rule"])
                except ValueError as e:
                    ap.error("--quant: %s" % e)
            if args.osd:
                lay.update(osd=True, osd_order=args.osd_order, osd_lambda=args.osd_lambda)
        if args.hard is not None:
            lay = dict(schedule="hard", hard_rule=C.BF_GRADIENT if args.hard == "gradient" else C.BF_THRESHOLD)
        if bsc is not None:
            from cuda_ldpc_amd.simulation import sweep_bsc
            if rank == 0:
                print("# %s N=%d K=%d, binary symmetric channel, bit flipping (%s rule), %s, maxIT=%d, batch=%d x %d GPU(s)%s" % (
                    os.path.basename(args.matrix), code.N, code.K, args.hard, "fixed iterations" if args.fixed else "per-frame early exit",
                    args.iters or 30, args.batch, world, ", random codewords (PN seed %d)" % args.pn_seed if args.pn_message else ""))
                print("#   P      NTF   NEF         FER         BER  AverIT       FER_F      FER_A")
            sweep_bsc(code, bsc, dist=dist, rule=lay["hard_rule"], Num_Frames_OneTime=args.batch, maxIT=args.iters or 30,
                      exit_mode=C.EXIT_FIXED if args.fixed else C.EXIT_PER_FRAME, max_batches=args.max_batches, displayStep=10 ** 12,
                      PN_Message=1 if args.pn_message else 0, pn_seed=args.pn_seed, log=print if rank == 0 else None)
            if world > 1:
                dist.destroy_process_group()
            return
        if bec is not None:
            from cuda_ldpc_amd.simulation import sweep_bec
            rm = C.RateMatch(code.N, shorten, puncture) if ratematch else None
            if rank == 0:
                print("# %s N=%d K=%d, binary erasure channel, %s, maxIT=%d, batch=%d x %d GPU(s)%s%s" % (
                    os.path.basename(args.matrix), code.N, code.K, "peeling + elimination" if args.ml else "peeling", args.iters or 100, args.batch,
                    world,
                    ", %d shortened, %d punctured, E=%d" % (rm.n_short, rm.n_punct, rm.E) if rm is not None else "",
                    ", random codewords (PN seed %d)" % args.pn_seed if args.pn_message else ""))
                print("#   P      NTF   NEF         FER         BER  AverIT       FER_F      FER_A")
            sweep_bec(code, bec, dist=dist, Num_Frames_OneTime=args.batch, maxIT=args.iters or 100, max_batches=args.max_batches, displayStep=10 ** 12,
                      PN_Message=1 if args.pn_message else 0, pn_seed=args.pn_seed, rate_match=rm, log=print if rank == 0 else None,
                      **(dict(ml=True, ml_max_erased=args.ml_max_erased) if args.ml else {}))
            if world > 1:
                dist.destroy_process_group()
            return
        mod = {}
        if args.qam != 2:  # the GF(q) half's constellation file and sigma (Eb/N0, n_QAM in the formula): the two sweeps share both
            mod = dict(n_QAM=args.qam, CONSTELLATION=C.Get_CONSTELLATION(os.path.join(nbd, "Constellation", "GRAY_%dQAM.txt" % args.qam), args.qam),
                       interleave=C.IL_ROWCOL if args.interleave == "rowcol" else C.IL_NONE)
        if args.harq is not None:
            from cuda_ldpc_amd.simulation import sweep_harq
            rvs = [C.RateMatch.circular(code.N, shorten, puncture, k0, E) for k0, E in harq]
            if rank == 0:
                print("# %s N=%d K=%d, HARQ over %s: buffer Ncb=%d (%d shortened, %d punctured), transmissions K0:E %s, first rate %.4f, %s, %s, "
                      "maxIT=%d, batch=%d x %d GPU(s)%s" % (os.path.basename(args.matrix), code.N, code.K,
                                                          "BPSK" if args.qam == 2 else "%d-QAM (Gray), interleaver %s" % (args.qam, args.interleave),
                                                          rvs[0].Ncb, rvs[0].n_short, rvs[0].n_punct,
                                                          args.harq, rvs[0].rate(code.K), "layered sum-product" if args.bp else
                                                          "quantised layered min-sum %r" % lay["quant"] if quant is not None else
                                                          "layered alpha=%g" % args.alpha if args.layered else
                                                          "flooding alpha=%g" % args.alpha, "fixed iterations" if args.fixed else "per-frame early exit",
                                                          args.iters or (25 if rows else 50), args.batch, world,
                                                          ", random codewords (PN seed %d)" % args.pn_seed if args.pn_message else "")
                      + (fade_words if fade is not None else "") + (", OSD-%d after the last transmission" % args.osd_order if args.osd else ""))
                print("# SNR      NTF  FER after each transmission ...  mean transmissions  throughput (information bits per bit sent)  AverIT"
                      + ("  OSD reprocessed correct" if args.osd else ""))
            sweep_harq(code, rvs, args.start, args.stop, args.step, snrtype=1 if args.snrtype is None else args.snrtype, dist=dist,
                       Num_Frames_OneTime=args.batch, maxIT=args.iters or (25 if rows else 50),
                       exit_mode=C.EXIT_FIXED if args.fixed else C.EXIT_PER_FRAME, max_batches=args.max_batches, PN_Message=1 if args.pn_message else 0,
                       pn_seed=args.pn_seed, log=print if rank == 0 else None, short_llr=args.short_llr, compact=not args.no_compact, **lay, **mod, **fad)
            if world > 1:
                dist.destroy_process_group()
            return
        if ratematch:
            rm = C.RateMatch(code.N, shorten, puncture)
            mod.update(rate_match=rm, short_llr=args.short_llr)
            if rank == 0:
                print("# rate matching: %d shortened, %d punctured, E=%d transmitted, rate (K - n_short) / E = %.4f" % (
                    rm.n_short, rm.n_punct, rm.E, rm.rate(code.K)))
        if rank == 0:
            print("# %s N=%d K=%d, %s%s%s, maxIT=%d, batch=%d x %d GPU(s)%s" % (os.path.basename(args.matrix), code.N, code.K,
                  "" if args.qam == 2 else "%d-QAM (Gray) %d bits per point, interleaver %s, max-log demapper, Eb/N0, " % (
                      args.qam, args.qam.bit_length() - 1, args.interleave),
                  "layered sum-product llr_scale=%s stop=%s, " % ("2/sigma^2" if args.qam == 2 else "1", stop) if args.bp else
                  "quantised layered min-sum %r stop=%s, " % (lay["quant"], stop) if quant is not None else
                  "layered min-sum alpha=%g stop=%s, " % (args.alpha, stop) if args.layered else
                  "hard decisions, bit flipping (%s rule), " % args.hard if args.hard is not None else
                  ("normalised flooding min-sum alpha=%g, " % args.alpha if args.alpha != 1.0 else ""),
                  "fixed iterations" if args.fixed else ("per-frame early exit" if args.per_frame else "batch-global early exit"),
                  args.iters or (25 if rows else 30 if args.hard is not None else 50), args.batch, world,
                  ", random codewords (PN seed %d, K'=%d), syndrome flag" % (args.pn_seed, code.K_info) if args.pn_message else "")
                  + (fade_words if fade is not None else "") + (", OSD-%d on the frames left with a non-zero syndrome" % args.osd_order if args.osd else ""))
            print("# SNR      NTF   NEF         FER         BER  AverIT       FER_F      FER_A" + ("  OSD reprocessed correct" if args.osd else ""))
        sweep(code, args.start, args.stop, args.step, snrtype=1 if args.qam == 2 else 0, dist=dist, Num_Frames_OneTime=args.batch, maxIT=args.iters or (25 if rows else 30 if args.hard is not None else 50),
              exit_mode=C.EXIT_FIXED if args.fixed else (C.EXIT_PER_FRAME if args.per_frame else C.EXIT_BATCH_GLOBAL), max_batches=args.max_batches, displayStep=10 ** 12, device_channel=args.device_channel,
              PN_Message=1 if args.pn_message else 0, pn_seed=args.pn_seed, log=print if rank == 0 else None, **lay, **mod, **fad)
    else:
        from cuda_ldpc_amd import nbldpc as nb
        from cuda_ldpc_amd.nb_simulation import sweep, sweep_harq
        mul, _, _ = nb.GFInitial(nb_q, os.path.join(nbd, "GF", "Arith.Table.GF.%d.txt" % nb_q))
        code = nb.NBCode(mpath, mul)
        bds = os.path.basename(mpath) == "BDS.576.288.GF.64.txt"
        # the one shipped codeword belongs to the BDS code; every other matrix sends the all-zero word unless --pn-message
        cw = np.loadtxt(os.path.join(nbd, "codeword_bds_gf64.txt"), dtype=np.int32) if bds else np.zeros(code.N, np.int32)
        con = None if args.qam == 2 else nb.Get_CONSTELLATION(os.path.join(nbd, "Constellation", "GRAY_%dQAM.txt" % args.qam), args.qam)
        if args.pn_message:
            words = ", random codewords (PN seed %d, K'=%d)" % (args.pn_seed, code.K_info)
        else:
            words = "" if bds else ", all-zero codeword"
        print("# %s N=%d symbols GF(%d), %s, maxIT=%d, %s%s" % (os.path.basename(mpath).replace(".txt", ""), code.N, code.q,
              ["EMS(2,2)", "trellis min-max", "log-QSPA = EMS(q,dc-1)", "layered trellis min-max", "FHT sum-product", "layered FHT sum-product"][args.method], args.iters or 20,
              "BPSK" if args.qam == 2 else "%d-QAM (Gray), one point per symbol" % args.qam, words) + (fade_words if fade is not None else ""))
        dev_ch = args.device_channel or fade is not None  # the fading channel exists on the device only
        nbatch = args.batch if dev_ch else min(args.batch, 1024)  # the host channel is serial: keep its batches small
        rmk = {}
        if ratematch:
            try:
                rvs = [C.RateMatch.circular(code.N, shorten, puncture, k0, E) for k0, E in harq] if args.harq is not None else [C.RateMatch(code.N, shorten, puncture)]
            except C._lib.LdpcError as e:
                ap.error(str(e))
            print("# rate matching over symbols: %d shortened, %d punctured, buffer Ncb=%d, E=%s transmitted, rate (K' - n_short) / E = %.4f" % (
                rvs[0].n_short, rvs[0].n_punct, rvs[0].Ncb, args.harq or rvs[0].E, (code.K_info - rvs[0].n_short) / rvs[0].E))
            rmk = dict(short_llr=args.short_llr)
        if args.harq is not None:
            print("# SNR      NTF  FER after each transmission ...  mean transmissions  throughput (information bits per bit sent)  AverIT")
            sweep_harq(code, rvs, cw, args.start, args.stop, args.step, snrtype=0 if args.snrtype is None else args.snrtype, maxIT=args.iters or 20,
                       batch=nbatch, max_batches=args.max_batches, decoder_method=args.method,
                       PN_Message=1 if args.pn_message else 0, pn_seed=args.pn_seed, compact=not args.no_compact, qspa_tier=args.qspa_tier, **rmk)
            return
        if ratematch:
            rmk["rate_match"] = rvs[0]
        print("# SNR      NTF   NEF         FER         BER  AverIT")
        sweep(code, cw, args.start, args.stop, args.step, maxIT=args.iters or 20, batch=nbatch,
              max_frames=None if args.max_batches is None else args.max_batches * nbatch, device_channel=dev_ch,
              decoder_method=args.method, n_QAM=args.qam, CONSTELLATION=con, PN_Message=1 if args.pn_message else 0, pn_seed=args.pn_seed,
              qspa_tier=args.qspa_tier, **fad, **rmk)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
