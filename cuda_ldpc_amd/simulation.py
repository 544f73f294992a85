"""Simulation_GPU and the Es/N0 sweep of the reference's binary program, driven through the C ABI.

Mirrors bldpc_实习/Simulation.cu:12-171 (batch loop: channel -> decode -> Statistic until the stop rule) and
main.cu:114-160 (sweep: seeds reset to 173/173/173 and counters cleared at every SNR point; SIM->SNR is a
float advanced by a double step).  Differences: shapes are arguments instead of define.cuh macros, the
statistics run on the device, and the batch may be sharded over ranks (sharding.py) with one all-reduce
of the counters per batch.
"""
import numpy as np
import torch

from . import sharding
from ._lib import check, lib
from .bldpc import (EXIT_BATCH_GLOBAL, EXIT_FIXED, EXIT_PER_FRAME, KERNEL_AUTO, STOP_PREFIX, STOP_SYNDROME, AWGNChannel_CPU, AWGNChannel_GPU,
                    AWGNChannel_QAM_GPU, AWGNChannel_RM_GPU, Decode_Statistic, Demodulate_QAM, LDPC_Decoder_GPU, LDPC_Decoder_Layered_GPU,
                    Modulate_QAM, PN_CodeWords, RM_Recover, RM_Select, SimCounters, Syndrome, _dev_ptr, sigma_of)
from .nbldpc import sigma_of as nb_sigma_of


def Simulation_GPU(code, seed, sigma, SIM, Num_Frames_OneTime=4096, maxIT=50, exit_mode=EXIT_BATCH_GLOBAL, kernel=KERNEL_AUTO,
                   leastErrorFrames=50, leastTestFrames=10000, displayStep=40960, dist=None, device=None, max_batches=None,
                   log=print, device_channel=False, PN_Message=0, pn_seed=0, schedule="flooding", alpha=1.0, stop_rule=None,
                   n_QAM=2, CONSTELLATION=None, rate_match=None, short_llr=1.0e4):
    """One SNR point (Simulation.cu:12-171).  `seed` (int32[3]) is the AWGN->seed state, advanced in place by the
    WHOLE batch on every rank so that all ranks stay on the reference's single noise stream.

    PN_Message=1 fills the reference's empty branch (Simulation.cu:107, define.cuh:26): every batch sends random
    codewords (bldpc_encode_random with stream `pn_seed`; frame b*F + i of the point is the same codeword at any world
    size), decodes them with a fixed iteration count, replaces the flag row of D by the syndrome check and counts errors
    against the sent CodeWord.  The flooding decoders' early exit assumes the zero word, so PN_Message=1 needs EXIT_FIXED there.

    schedule="flooding" with alpha != 1.0 decodes with the normalised flooding kernels (LDPC_Decoder_GPU(alpha=alpha)): EXIT_FIXED or
    EXIT_PER_FRAME; PN_Message=1 still needs EXIT_FIXED, the prefix rule tests for the zero word.

    schedule="layered" decodes with LDPC_Decoder_Layered_GPU (normalisation factor `alpha`; EXIT_FIXED or EXIT_PER_FRAME, `kernel`
    is not used).  stop_rule defaults to STOP_SYNDROME with PN_Message=1 and to STOP_PREFIX otherwise; with STOP_SYNDROME the flag
    row already means "valid codeword", so random codewords run with EXIT_PER_FRAME and no separate Syndrome call.

    n_QAM != 2 sends the codewords over n_QAM-QAM instead of BPSK: CONSTELLATION (host float32 [n_QAM, 2], Get_CONSTELLATION) labels
    log2(n_QAM) consecutive codeword bits per point; a batch is encode -> Modulate_QAM -> AWGNChannel_QAM_GPU (four draws per symbol
    of the same noise stream) -> Demodulate_QAM with scale 1 / (2 sigma^2) -> the chosen decoder, and the caller passes the sigma of
    that n_QAM (nbldpc.sigma_of).  Needs PN_Message=1 (a QAM channel is not symmetric) and device_channel=True.

    rate_match (a RateMatch over code.N) simulates the shortened and punctured code: only its E transmitted bits go over the channel,
    2 E draws per frame (4 ceil(E / m) over QAM), and the decoder's input is short_llr on the shortened positions and +0.0 on the punctured
    ones.  BPSK: the fused channel AWGNChannel_RM_GPU.  QAM: RM_Select -> Modulate_QAM with E bits -> channel -> Demodulate_QAM with E ->
    RM_Recover.  Random codewords keep the shortened bits 0 (PN_CodeWords(rate_match=...)).  The decoder and Statistic calls, `length`
    included, are those of the mother code: a shortened bit inside the prefix is 0 on both sides and adds no error; the printed BER divides
    by the prefix bits that are not shortened.  The caller passes the sigma of the derived rate, rate_match.rate(code.K).  Needs
    device_channel=True."""
    if PN_Message not in (0, 1):
        raise ValueError("PN_Message must be 0 (all-zero codeword) or 1 (random codewords)")
    if schedule not in ("flooding", "layered"):
        raise ValueError("schedule must be 'flooding' or 'layered'")
    layered = schedule == "layered"
    if not layered and stop_rule is not None:
        raise ValueError("stop_rule belongs to schedule='layered'")
    norm = not layered and alpha != 1.0  # normalised min-sum on the flooding decoders (LDPC_Decoder_GPU(alpha=...))
    if norm and exit_mode not in (EXIT_FIXED, EXIT_PER_FRAME):
        raise ValueError("schedule='flooding' with alpha takes EXIT_FIXED or EXIT_PER_FRAME")
    if layered:
        if stop_rule is None:
            stop_rule = STOP_SYNDROME if PN_Message else STOP_PREFIX
        if stop_rule not in (STOP_PREFIX, STOP_SYNDROME):
            raise ValueError("stop_rule must be STOP_PREFIX or STOP_SYNDROME")
        if exit_mode not in (EXIT_FIXED, EXIT_PER_FRAME):
            raise ValueError("schedule='layered' takes EXIT_FIXED or EXIT_PER_FRAME")
        if PN_Message == 1 and stop_rule != STOP_SYNDROME and exit_mode != EXIT_FIXED:
            raise ValueError("PN_Message=1 with per-frame exit needs stop_rule=STOP_SYNDROME: STOP_PREFIX tests for the all-zero word")
    elif PN_Message == 1 and exit_mode != EXIT_FIXED:
        raise ValueError("PN_Message=1 needs exit_mode=EXIT_FIXED: the decoders' early exit tests for the all-zero word")
    qam_m = 0
    if n_QAM != 2:  # every refusal before anything touches the device
        if PN_Message != 1:
            raise ValueError("n_QAM=%r needs PN_Message=1: a QAM channel is not symmetric in the bits, so the all-zero word (always the "
                             "same constellation point) is not representative of a random codeword" % (n_QAM,))
        if not device_channel:
            raise ValueError("n_QAM != 2 needs device_channel=True: there is no host QAM channel on this path")
        if CONSTELLATION is None:
            raise ValueError("n_QAM=%r needs CONSTELLATION (float32 [n_QAM, 2], Get_CONSTELLATION)" % (n_QAM,))
        con = np.ascontiguousarray(CONSTELLATION, np.float32)
        if not isinstance(n_QAM, (int, np.integer)) or n_QAM < 2 or n_QAM > 256 or n_QAM & (n_QAM - 1) or con.shape != (n_QAM, 2):
            raise ValueError("CONSTELLATION must be float32 [n_QAM, 2] with n_QAM a power of two in 2..256, not %s for n_QAM=%r"
                             % (con.shape, n_QAM))
        qam_m = int(n_QAM).bit_length() - 1
    elif CONSTELLATION is not None:
        raise ValueError("CONSTELLATION belongs to n_QAM != 2")
    rm = rate_match
    if rm is not None:
        if not device_channel:
            raise ValueError("rate_match needs device_channel=True: the rate-matched sweep runs on the device channel")
        if rm.N != code.N:
            raise ValueError("rate_match is over N=%d positions, the code has N=%d" % (rm.N, code.N))
        if not (np.isfinite(short_llr) and short_llr > 0):
            raise ValueError("short_llr must be finite and > 0, not %r" % (short_llr,))
        # code.info_positions builds the code's generator on first use, as the first batch of random codewords would
        if PN_Message and rm.n_short and not np.isin(rm.shorten, code.info_positions).all():
            raise ValueError("rate_match shortens a parity position of the code's generator; only information positions (code.info_positions) "
                             "can be agreed to be 0")
    rank = dist.get_rank() if dist is not None and dist.is_initialized() else 0
    world = dist.get_world_size() if dist is not None and dist.is_initialized() else 1
    device = device or torch.device("cuda", torch.cuda.current_device())
    F = Num_Frames_OneTime
    first, count = sharding.shard_frames(F, world, rank)
    n_tx = rm.E if rm is not None else code.N  # bits per frame that go over the channel
    per_frame = sharding.qam_draws_per_frame(n_tx, qam_m) if qam_m else sharding.binary_draws_per_frame(n_tx)
    con_dev = torch.from_numpy(con).to(device) if qam_m else None
    dev_cnt = torch.zeros(5, dtype=torch.int64, device=device)
    D = torch.empty((code.N + 1, max(count, 1)), dtype=torch.int32, device=device)
    length = code.K  # Message_CW 0 (define.cuh:61)
    ber_bits = length - (int((rm.shorten < length).sum()) if rm is not None else 0)  # the prefix bits that carry information
    batches = 0
    while True:
        SIM.num_Frames += F  # Simulation.cu:113
        my_seed = sharding.lcg_jump(seed, first * per_frame)
        cw = PN_CodeWords(code, pn_seed, count, first_frame=batches * F + first, device=device, rate_match=rm) if (PN_Message and count) else None
        if not count:
            yd = None
        elif rm is not None and qam_m:  # the modem sees the E transmitted bits only
            rx = AWGNChannel_QAM_GPU(my_seed, sigma, Modulate_QAM(RM_Select(rm, cw), rm.E, qam_m), con_dev)
            yd = RM_Recover(rm, Demodulate_QAM(rx, con_dev, 1.0 / (2.0 * sigma * sigma), rm.E), short_llr)
        elif rm is not None:
            yd = AWGNChannel_RM_GPU(rm, my_seed, sigma, count, device=device, CodeWord=cw, short_llr=short_llr)
        elif qam_m:  # bits -> points -> noisy points -> max-log LLRs, all on the device
            rx = AWGNChannel_QAM_GPU(my_seed, sigma, Modulate_QAM(cw, code.N, qam_m), con_dev)
            yd = Demodulate_QAM(rx, con_dev, 1.0 / (2.0 * sigma * sigma), code.N)
        elif device_channel:  # same draws, generated on the GPU (device libm in the Box-Muller transform)
            yd = AWGNChannel_GPU(my_seed, sigma, code.N, count, device=device, CodeWord=cw)
        else:
            yd = torch.from_numpy(AWGNChannel_CPU(my_seed, sigma, code.N, count, CodeWord=None if cw is None else cw.cpu().numpy())).to(device)
        seed[:] = sharding.lcg_jump(seed, F * per_frame)
        dev_cnt.zero_()
        if count and layered:
            r = LDPC_Decoder_Layered_GPU(code, yd, max_iter=maxIT, alpha=alpha, length=length, exit_mode=exit_mode, stop_rule=stop_rule, D=D)
            if PN_Message and stop_rule != STOP_SYNDROME:
                Syndrome(code, D, into_flag_row=True)
            st = torch.cuda.current_stream(device).cuda_stream
            check(lib.bldpc_statistic_per_frame(code._h, _dev_ptr(D), _dev_ptr(cw), count, length, _dev_ptr(r["iters"]), _dev_ptr(dev_cnt), st),
                  "Statistic")
        elif count and (PN_Message or norm):
            r = LDPC_Decoder_GPU(code, yd, max_iter=maxIT, length=length, exit_mode=exit_mode, kernel=kernel, D=D, alpha=alpha if norm else None)
            if PN_Message:
                Syndrome(code, D, into_flag_row=True)  # flag row: "valid codeword" instead of "first `length` bits zero"
            st = torch.cuda.current_stream(device).cuda_stream
            if r.get("iters") is not None:
                check(lib.bldpc_statistic_per_frame(code._h, _dev_ptr(D), _dev_ptr(cw), count, length, _dev_ptr(r["iters"]), _dev_ptr(dev_cnt), st),
                      "Statistic")
            else:
                check(lib.bldpc_statistic(code._h, _dev_ptr(D), _dev_ptr(cw), count, length, r["iteraTime"], _dev_ptr(dev_cnt), st), "Statistic")
        elif count:
            Decode_Statistic(code, yd, dev_cnt, max_iter=maxIT, length=length, exit_mode=exit_mode, kernel=kernel, D=D)  # Simulation.cu:143-145
        sharding.allreduce_counters(dev_cnt, dist)
        c = dev_cnt.cpu().tolist()
        SIM.num_Error_Frames += c[0]
        SIM.num_Error_Bits += c[1]
        SIM.Total_Iteration += c[2]
        SIM.num_False_Frames += c[3]
        SIM.num_Alarm_Frames += c[4]
        batches += 1
        stop = SIM.num_Error_Frames >= leastErrorFrames and SIM.num_Frames >= leastTestFrames
        last = max_batches is not None and batches >= max_batches
        if rank == 0 and log and (SIM.num_Frames % displayStep == 0 or stop or last):
            log(format_row(SIM, ber_bits))
        if stop or (max_batches is not None and batches >= max_batches):
            return 1 if stop else 0


def format_row(SIM, length):
    """The reference's result row (Simulation.cu:272): SNR NTF NEF FER BER AverIT FER_F FER_A."""
    r = SIM.ratios(length)
    return " %.1f %8d  %4d  %6.4e  %6.4e  %.2f  %6.4e %6.4e" % (SIM.SNR, SIM.num_Frames, SIM.num_Error_Frames, r["FER"], r["BER"],
                                                           r["AverageIT"], r["FER_False"], r["FER_Alarm"])


def snr_grid(startSNR=0.0, stopSNR=13.0, stepSNR=0.2):
    """SNR points the reference visits: a float32 accumulated with a double step (main.cu:114)."""
    pts, s = [], np.float32(startSNR)
    while s <= stopSNR:
        pts.append(float(s))
        s = np.float32(np.float64(s) + stepSNR)
    return pts


def sweep(code, startSNR=0.0, stopSNR=13.0, stepSNR=0.2, snrtype=1, seeds=(173, 173, 173), dist=None, log=print, n_QAM=2, **kw):
    """main.cu:114-160: returns the list of SimCounters, one per SNR point.  With n_QAM != 2 (pass the constellation itself as
    CONSTELLATION=...) the sigma of a point is the GF(q) program's, nbldpc_sigma(SNR, snrtype, n_QAM, rate), so that a binary and a
    GF(q) sweep of the same rate, snrtype and n_QAM run at the same sigma at every SNR value.  With rate_match=rm the rate in either
    formula is the derived code's, rm.rate(code.K) (it enters when snrtype is Eb/N0)."""
    out = []
    rate = kw["rate_match"].rate(code.K) if kw.get("rate_match") is not None else code.K / code.N
    if n_QAM != 2:
        kw["n_QAM"] = n_QAM
    for snr in snr_grid(startSNR, stopSNR, stepSNR):
        seed = np.array(seeds, np.int32)  # reset at every point (main.cu:117-119)
        SIM = SimCounters()
        SIM.SNR = snr
        sigma = nb_sigma_of(snr, rate, snrtype, n_QAM) if n_QAM != 2 else sigma_of(snr, snrtype, rate)
        Simulation_GPU(code, seed, sigma, SIM, dist=dist, log=log, **kw)
        out.append(SIM)
    return out
