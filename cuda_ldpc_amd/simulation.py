"""Simulation_GPU and the Es/N0 sweep of the reference's binary program, driven through the C ABI.

Mirrors bldpc_实习/Simulation.cu:12-171 (batch loop: channel -> decode -> Statistic until the stop rule) and
main.cu:114-160 (sweep: seeds reset to 173/173/173 and counters cleared at every SNR point; SIM->SNR is a
float advanced by a double step).  Differences: shapes are arguments instead of define.cuh macros, the
statistics run on the device, and the batch may be sharded over ranks (sharding.py) with one all-reduce
of the counters per batch.
"""
from dataclasses import dataclass, field

import numpy as np
import torch

from . import sharding
from ._lib import check, lib
from .bldpc import (BF_GRADIENT, BF_THRESHOLD, BSCChannel_GPU, Hard_Pack, LDPC_Decoder_BitFlip_GPU,
                    BECChannel_GPU, Hard_Pack_Int, LDPC_Decoder_Erasure_GPU, LDPC_Decoder_Erasure_ML_GPU, RM_Recover_Bits, RM_Select_Bits, Statistic_Bits,
                    EXIT_BATCH_GLOBAL, EXIT_FIXED, EXIT_PER_FRAME, KERNEL_AUTO, STOP_PREFIX, STOP_SYNDROME, AWGNChannel_CPU, AWGNChannel_Fading_GPU,
                    AWGNChannel_GPU, AWGNChannel_QAM_Fading_GPU, AWGNChannel_QAM_GPU, AWGNChannel_RM_Combine_GPU, AWGNChannel_RM_GPU,
                    Decode_Statistic, Demodulate_QAM, Demodulate_QAM_Fading, Fading, Fading_Gains, Frames_Gather, Frames_Scatter, IL_NONE, IL_ROWCOL,
                    LDPC_Decoder_BP_GPU, LDPC_Decoder_GPU, LDPC_Decoder_Layered_GPU, LDPC_Decoder_OSD_GPU, LDPC_Decoder_Quant_GPU, Modulate_QAM, PN_CodeWords, Quant,
                    RM_Combine, RM_Demodulate_QAM_Recover, RM_Modulate_QAM, RM_Recover, RM_Select, SimCounters, Syndrome, _dev_ptr, sigma_of)
from .nbldpc import sigma_of as nb_sigma_of


def _check_schedule(schedule, alpha, quant):
    """The schedule of a sweep against its alpha and quant, as Simulation_GPU and Simulation_HARQ_GPU both refuse them.  Returns
    (bp, layered): sum-product, any of the row-layered decoders."""
    if schedule not in ("flooding", "layered", "bp", "quant", "hard"):
        raise ValueError("schedule must be 'flooding', 'layered', 'bp', 'quant' or 'hard'")
    if schedule == "hard" and (alpha != 1.0 or quant is not None):
        raise ValueError("schedule='hard' decodes hard decisions by bit flipping: it has no alpha and no quant")
    bp = schedule == "bp"
    layered = schedule in ("layered", "bp", "quant")  # the row-layered decoders share modes, rules and outputs
    if bp and alpha != 1.0:
        raise ValueError("alpha belongs to the min-sum decoders: schedule='bp' has no normalisation factor")
    if (schedule == "quant") != (quant is not None) or not isinstance(quant, (Quant, type(None))):
        raise ValueError("schedule='quant' needs quant (a Quant), and quant belongs to schedule='quant'")
    if quant is not None and alpha != 1.0:
        raise ValueError("schedule='quant' takes its correction from quant.norm8 and quant.offset, not from alpha")
    return bp, layered


def _check_osd(osd, schedule, stop_rule, osd_order=0, osd_lambda=0):
    """osd=True against the schedule and the resolved stop rule, as Simulation_GPU and Simulation_HARQ_GPU both refuse it; osd_order
    and osd_lambda (bldpc_decode_osd_w) belong to osd=True."""
    if not osd:
        if osd_order or osd_lambda:
            raise ValueError("osd_order and osd_lambda belong to osd=True")
        return
    if osd_order not in (0, 1, 2) or int(osd_lambda) != osd_lambda or osd_lambda < 0:
        raise ValueError("osd_order must be 0, 1 or 2 and osd_lambda a non-negative integer")
    if schedule not in ("layered", "bp", "quant"):
        raise ValueError("osd belongs to schedule='layered', schedule='bp' and schedule='quant': reprocessing orders the positions by a "
                         "decoder's a-posteriori values")
    if stop_rule != STOP_SYNDROME:
        raise ValueError("osd needs stop_rule=STOP_SYNDROME: the frames to reprocess are those whose flag says 'no codeword'")


def _osd_reprocess(code, D, app, cw, osd_cnt, osd_order=0, osd_lambda=0):
    """LDPC_Decoder_OSD_GPU on a decoder's D (in place) and app (a quantised app converted to float, which is exact); adds the frames
    reprocessed and those of them that came out equal to the word sent to osd_cnt (CUDA int64 [2])."""
    flips = LDPC_Decoder_OSD_GPU(code, app if app.dtype == torch.float32 else app.float(), D=D, order=osd_order, lam=osd_lambda)[1]
    done = flips >= 0
    same = ~((D[:code.N] != cw) if cw is not None else (D[:code.N] != 0)).any(0)
    osd_cnt[0] += done.sum()
    osd_cnt[1] += (done & same).sum()


def _check_qam(n_QAM, CONSTELLATION, PN_Message, interleave):
    """The QAM arguments of a sweep, as Simulation_GPU and Simulation_HARQ_GPU both refuse them, before anything touches the device.
    Returns (bits per symbol or 0 for BPSK, the constellation as a host float32 [n_QAM, 2] or None)."""
    if interleave not in (IL_NONE, IL_ROWCOL):
        raise ValueError("interleave must be IL_NONE (0) or IL_ROWCOL (1), not %r" % (interleave,))
    if n_QAM == 2:
        if CONSTELLATION is not None:
            raise ValueError("CONSTELLATION belongs to n_QAM != 2")
        if interleave != IL_NONE:
            raise ValueError("interleave belongs to n_QAM != 2: the BPSK channel has one bit per symbol and nothing to interleave")
        return 0, None
    if PN_Message != 1:
        raise ValueError("n_QAM=%r needs PN_Message=1: a QAM channel is not symmetric in the bits, so the all-zero word (always the "
                         "same constellation point) is not representative of a random codeword" % (n_QAM,))
    if CONSTELLATION is None:
        raise ValueError("n_QAM=%r needs CONSTELLATION (float32 [n_QAM, 2], Get_CONSTELLATION)" % (n_QAM,))
    con = np.ascontiguousarray(CONSTELLATION, np.float32)
    if not isinstance(n_QAM, (int, np.integer)) or n_QAM < 2 or n_QAM > 256 or n_QAM & (n_QAM - 1) or con.shape != (n_QAM, 2):
        raise ValueError("CONSTELLATION must be float32 [n_QAM, 2] with n_QAM a power of two in 2..256, not %s for n_QAM=%r"
                         % (con.shape, n_QAM))
    return int(n_QAM).bit_length() - 1, con


def _check_fading(fading, device_channel, exit_mode):
    """The fading argument of a sweep, as the three drivers refuse it before anything touches the device."""
    if fading is None:
        return
    if not isinstance(fading, Fading):
        raise ValueError("fading must be a Fading (block length and the seed of the fading stream), not %r" % (fading,))
    if not device_channel:
        raise ValueError("fading needs device_channel=True: the gains and the channels that apply them run on the device")
    if exit_mode == EXIT_BATCH_GLOBAL:
        raise ValueError("fading takes EXIT_FIXED or EXIT_PER_FRAME: the results of EXIT_BATCH_GLOBAL depend on the batch")
    fading.check()


def _fading_gains(fading, S, F, first, count, device):
    """The gains of this rank's `count` frames (global frames first .. first + count - 1 of a batch of F) for one transmission of S
    channel uses, CUDA float32 [count, S] (None without frames), and the fading seed advanced by the WHOLE batch, as the noise seed is."""
    per_frame = sharding.fading_draws_per_frame(S, fading.Lc)
    my_seed = sharding.lcg_jump(fading.seed, first * per_frame)
    fading.seed[:] = sharding.lcg_jump(fading.seed, F * per_frame)
    return Fading_Gains(my_seed, fading.Lc, S, count, device=device) if count else None


def _fading_transmit(fading_gain, my_seed, sigma, cw, n_bits, count, qam_m, con_dev, interleave, rm=None):
    """One transmission over the fading channel as the composition include/bldpc.h names: the matched-filter values (BPSK) or max-log
    values with CSI (QAM) of the n_bits transmitted bits, CUDA float32 [n_bits, count].  rm: the profile that selects them from cw."""
    if qam_m:
        sym = RM_Modulate_QAM(rm, cw, qam_m, interleave=interleave) if rm is not None else Modulate_QAM(cw, n_bits, qam_m, interleave=interleave)
        rx = AWGNChannel_QAM_Fading_GPU(my_seed, sigma, sym, con_dev, fading_gain)
        return Demodulate_QAM_Fading(rx, fading_gain, con_dev, 1.0 / (2.0 * sigma * sigma), n_bits, interleave=interleave)
    tx = RM_Select(rm, cw) if (rm is not None and cw is not None) else cw
    return AWGNChannel_Fading_GPU(my_seed, sigma, fading_gain, n_bits, count, CodeWord=tx)


def _qam_receive(rm, rx, con_dev, scale, short_llr, interleave, acc=None, done=None):
    """The decoder input of one rate-matched transmission over QAM: recover (acc None) or combine into acc under done.  The fused
    call and its two-call composition give the same bits; which one runs follows profiles/harq_qam_time.txt: the fused
    recover is the faster one at one lap of the buffer (0.75 to 0.97 of the composition), everything else is not (a combine with no
    whole wavefront of done frames 1.00 to 1.21, two laps 1.17 to 1.98)."""
    if acc is None and rm.laps == 1:
        return RM_Demodulate_QAM_Recover(rm, rx, con_dev, scale, short_llr, interleave=interleave)
    llr = Demodulate_QAM(rx, con_dev, scale, rm.E, interleave=interleave)
    if acc is None:
        return RM_Recover(rm, llr, short_llr)
    return RM_Combine(rm, llr, acc, done=done, short_llr=short_llr)


def Simulation_GPU(code, seed, sigma, SIM, Num_Frames_OneTime=4096, maxIT=50, exit_mode=EXIT_BATCH_GLOBAL, kernel=KERNEL_AUTO,
                   leastErrorFrames=50, leastTestFrames=10000, displayStep=40960, dist=None, device=None, max_batches=None,
                   log=print, device_channel=False, PN_Message=0, pn_seed=0, schedule="flooding", alpha=1.0, stop_rule=None,
                   n_QAM=2, CONSTELLATION=None, rate_match=None, short_llr=1.0e4, quant=None, interleave=IL_NONE, fading=None, hard_rule=None,
                   osd=False, osd_order=0, osd_lambda=0):
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

    schedule="bp" decodes with LDPC_Decoder_BP_GPU (layered sum-product): everything said of schedule="layered" holds, except that
    `alpha` is refused (sum-product has no normalisation factor) and that the decoder is given llr_scale = 2 / sigma^2 on the BPSK paths,
    rate-matched included, which turns y = 1 - 2c + noise into a true LLR, and 1.0 on the QAM paths, whose demapper already scales by
    1 / (2 sigma^2).

    schedule="quant" decodes with LDPC_Decoder_Quant_GPU (layered min-sum with the finite word lengths of `quant`, a Quant): everything
    said of schedule="layered" holds, except that `alpha` is refused (quant.norm8 and quant.offset are the correction) and that the
    decoder's input, whatever channel, modem or rate matching made it, goes through the quantiser with the gain quant.llr_scale.

    n_QAM != 2 sends the codewords over n_QAM-QAM instead of BPSK: CONSTELLATION (host float32 [n_QAM, 2], Get_CONSTELLATION) labels
    log2(n_QAM) consecutive codeword bits per point; a batch is encode -> Modulate_QAM -> AWGNChannel_QAM_GPU (four draws per symbol
    of the same noise stream) -> Demodulate_QAM with scale 1 / (2 sigma^2) -> the chosen decoder, and the caller passes the sigma of
    that n_QAM (nbldpc.sigma_of).  Needs PN_Message=1 (a QAM channel is not symmetric) and device_channel=True.  interleave=IL_ROWCOL
    puts the row-column bit interleaver between the bits and the points (the modem's index rule, include/bldpc.h); it belongs to
    n_QAM != 2.

    rate_match (a RateMatch over code.N) simulates the shortened and punctured code: only its E transmitted bits go over the channel,
    2 E draws per frame (4 ceil(E / m) over QAM), and the decoder's input is short_llr on the shortened positions and +0.0 on the punctured
    ones.  BPSK: the fused channel AWGNChannel_RM_GPU.  QAM: RM_Modulate_QAM -> channel -> RM_Demodulate_QAM_Recover, the bits of
    RM_Select -> Modulate_QAM with E bits -> channel -> Demodulate_QAM with E -> RM_Recover without the two [E, F] arrays.  Random
    codewords keep the shortened bits 0 (PN_CodeWords(rate_match=...)).  The decoder and Statistic calls, `length` included, are those of
    the mother code: a shortened bit inside the prefix is 0 on both sides and adds no error; the printed BER divides
    by the prefix bits that are not shortened.  The caller passes the sigma of the derived rate, rate_match.rate(code.K).  Needs
    device_channel=True.

    schedule="hard" decodes the hard decisions of the channel values with LDPC_Decoder_BitFlip_GPU (rule `hard_rule`, BF_GRADIENT by
    default; `hard_rule` belongs to this schedule): whatever chain makes Channel_Out (BPSK, QAM, fading) is followed by Hard_Pack and the
    decoder, EXIT_FIXED or EXIT_PER_FRAME.  Its flag is always the syndrome, so random codewords run with either exit mode.  `alpha`,
    `quant`, `stop_rule` and `rate_match` are refused: a punctured position is an erasure, and a hard decoder has no value for it.

    fading (a Fading) puts flat Rayleigh block fading with receiver CSI on the channel (include/bldpc.h, "block fading"): every batch
    draws the gains of its S channel uses per frame (S = the transmitted bits over BPSK, ceil(bits / m) points over QAM) from the fading
    stream, fading.seed, which is advanced in place by the whole batch on every rank, ceil(S / Lc) draws per frame, while the noise
    stream and its draws stay what they are without fading.  BPSK: AWGNChannel_Fading_GPU (a * r, so that 2 / sigma^2 stays the
    sum-product scale); QAM: AWGNChannel_QAM_Fading_GPU -> Demodulate_QAM_Fading; with rate_match the compositions RM_Select ->
    channel at E -> RM_Recover and RM_Modulate_QAM -> channel -> Demodulate_QAM_Fading at E -> RM_Recover.  E[a^2] = 1, so the caller
    passes the sigma of the AWGN sweep.  Needs device_channel=True and EXIT_FIXED or EXIT_PER_FRAME; fading=None is the AWGN sweep,
    call for call.

    osd=True ("BP + OSD") sends the decoder's D and app through LDPC_Decoder_OSD_GPU before the statistics: the frames the decoder left
    with a non-zero syndrome are reprocessed (ordered statistics of order 0, include/bldpc.h) and come out codewords with flag 1; the
    iteration counts stay the decoder's.  schedule 'layered', 'bp' or 'quant' with stop_rule=STOP_SYNDROME; refused elsewhere.
    SIM.num_OSD_Frames counts the frames reprocessed and SIM.num_OSD_Correct those of them that came out equal to the word sent; the
    log row ends with both.  osd_order = 1 or 2 with osd_lambda (bldpc_decode_osd_w): the reprocessing also tries every single trusted
    position flipped and, at order 2, the pairs among the osd_lambda least reliable of them; an error without osd=True."""
    if PN_Message not in (0, 1):
        raise ValueError("PN_Message must be 0 (all-zero codeword) or 1 (random codewords)")
    bp, layered = _check_schedule(schedule, alpha, quant)
    hard = schedule == "hard"
    if not layered and stop_rule is not None:
        raise ValueError("stop_rule belongs to schedule='layered', schedule='bp' and schedule='quant'")
    if hard_rule is not None and not hard:
        raise ValueError("hard_rule belongs to schedule='hard'")
    if hard:
        hard_rule = BF_GRADIENT if hard_rule is None else hard_rule
        if hard_rule not in (BF_THRESHOLD, BF_GRADIENT):
            raise ValueError("hard_rule must be BF_THRESHOLD or BF_GRADIENT")
        if rate_match is not None:
            raise ValueError("schedule='hard' takes no rate_match: punctured positions are erasures, and a hard decoder has no value for them")
        if exit_mode not in (EXIT_FIXED, EXIT_PER_FRAME):
            raise ValueError("schedule='hard' takes EXIT_FIXED or EXIT_PER_FRAME")
    norm = not layered and alpha != 1.0  # normalised min-sum on the flooding decoders (LDPC_Decoder_GPU(alpha=...))
    if norm and exit_mode not in (EXIT_FIXED, EXIT_PER_FRAME):
        raise ValueError("schedule='flooding' with alpha takes EXIT_FIXED or EXIT_PER_FRAME")
    if layered:
        if stop_rule is None:
            stop_rule = STOP_SYNDROME if PN_Message else STOP_PREFIX
        if stop_rule not in (STOP_PREFIX, STOP_SYNDROME):
            raise ValueError("stop_rule must be STOP_PREFIX or STOP_SYNDROME")
        if exit_mode not in (EXIT_FIXED, EXIT_PER_FRAME):
            raise ValueError("schedule='%s' takes EXIT_FIXED or EXIT_PER_FRAME" % schedule)
        if PN_Message == 1 and stop_rule != STOP_SYNDROME and exit_mode != EXIT_FIXED:
            raise ValueError("PN_Message=1 with per-frame exit needs stop_rule=STOP_SYNDROME: STOP_PREFIX tests for the all-zero word")
    elif PN_Message == 1 and exit_mode != EXIT_FIXED and not hard:
        raise ValueError("PN_Message=1 needs exit_mode=EXIT_FIXED: the decoders' early exit tests for the all-zero word")
    if n_QAM != 2 and PN_Message == 1 and not device_channel:  # every refusal before anything touches the device
        raise ValueError("n_QAM != 2 needs device_channel=True: there is no host QAM channel on this path")
    _check_osd(osd, schedule, stop_rule, osd_order, osd_lambda)
    qam_m, con = _check_qam(n_QAM, CONSTELLATION, PN_Message, interleave)
    _check_fading(fading, device_channel, exit_mode)
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
    osd_cnt = torch.zeros(2, dtype=torch.int64, device=device) if osd else None  # frames reprocessed, and of them equal to the word sent
    D = torch.empty((code.N + 1, max(count, 1)), dtype=torch.int32, device=device)
    length = code.K  # Message_CW 0 (define.cuh:61)
    llr_scale = 1.0 if qam_m else 2.0 / (sigma * sigma)  # schedule="bp": what makes the decoder's input a true LLR
    ber_bits = length - (int((rm.shorten < length).sum()) if rm is not None else 0)  # the prefix bits that carry information
    batches = 0
    while True:
        SIM.num_Frames += F  # Simulation.cu:113
        my_seed = sharding.lcg_jump(seed, first * per_frame)
        cw = PN_CodeWords(code, pn_seed, count, first_frame=batches * F + first, device=device, rate_match=rm) if (PN_Message and count) else None
        if fading is not None:  # the gains of this batch, then the composition of the header over them
            gain = _fading_gains(fading, sharding.fading_uses(n_tx, qam_m), F, first, count, device)
        if not count:
            yd = None
        elif fading is not None:
            yd = _fading_transmit(gain, my_seed, sigma, cw, n_tx, count, qam_m, con_dev, interleave, rm)
            if rm is not None:
                yd = RM_Recover(rm, yd, short_llr)
        elif rm is not None and qam_m:  # the modem sees the E transmitted bits only
            rx = AWGNChannel_QAM_GPU(my_seed, sigma, RM_Modulate_QAM(rm, cw, qam_m, interleave=interleave), con_dev)
            yd = _qam_receive(rm, rx, con_dev, 1.0 / (2.0 * sigma * sigma), short_llr, interleave)
        elif rm is not None:
            yd = AWGNChannel_RM_GPU(rm, my_seed, sigma, count, device=device, CodeWord=cw, short_llr=short_llr)
        elif qam_m:  # bits -> points -> noisy points -> max-log LLRs, all on the device
            rx = AWGNChannel_QAM_GPU(my_seed, sigma, Modulate_QAM(cw, code.N, qam_m, interleave=interleave), con_dev)
            yd = Demodulate_QAM(rx, con_dev, 1.0 / (2.0 * sigma * sigma), code.N, interleave=interleave)
        elif device_channel:  # same draws, generated on the GPU (device libm in the Box-Muller transform)
            yd = AWGNChannel_GPU(my_seed, sigma, code.N, count, device=device, CodeWord=cw)
        else:
            yd = torch.from_numpy(AWGNChannel_CPU(my_seed, sigma, code.N, count, CodeWord=None if cw is None else cw.cpu().numpy())).to(device)
        seed[:] = sharding.lcg_jump(seed, F * per_frame)
        dev_cnt.zero_()
        if osd:
            osd_cnt.zero_()
        if count and hard:
            r = LDPC_Decoder_BitFlip_GPU(code, Hard_Pack(yd), count, rule=hard_rule, max_iter=maxIT, exit_mode=exit_mode, D=D)
            st = torch.cuda.current_stream(device).cuda_stream
            check(lib.bldpc_statistic_per_frame(code._h, _dev_ptr(D), _dev_ptr(cw), count, length, _dev_ptr(r["iters"]), _dev_ptr(dev_cnt), st),
                  "Statistic")
        elif count and layered:
            if bp:
                r = LDPC_Decoder_BP_GPU(code, yd, max_iter=maxIT, llr_scale=llr_scale, length=length, exit_mode=exit_mode, stop_rule=stop_rule, D=D,
                                        want_app=osd)
            elif quant is not None:
                r = LDPC_Decoder_Quant_GPU(code, yd, quant, max_iter=maxIT, length=length, exit_mode=exit_mode, stop_rule=stop_rule, D=D,
                                           want_app=osd)
            else:
                r = LDPC_Decoder_Layered_GPU(code, yd, max_iter=maxIT, alpha=alpha, length=length, exit_mode=exit_mode, stop_rule=stop_rule, D=D,
                                             want_app=osd)
            if PN_Message and stop_rule != STOP_SYNDROME:
                Syndrome(code, D, into_flag_row=True)
            if osd:
                _osd_reprocess(code, D, r["app"], cw, osd_cnt, osd_order, osd_lambda)
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
        if osd:
            o = sharding.allreduce_counters(osd_cnt, dist).cpu().tolist()
            SIM.num_OSD_Frames += o[0]
            SIM.num_OSD_Correct += o[1]
        batches += 1
        stop = SIM.num_Error_Frames >= leastErrorFrames and SIM.num_Frames >= leastTestFrames
        last = max_batches is not None and batches >= max_batches
        if rank == 0 and log and (SIM.num_Frames % displayStep == 0 or stop or last):
            log(format_row(SIM, ber_bits) + ("  OSD %d %d" % (SIM.num_OSD_Frames, SIM.num_OSD_Correct) if osd else ""))
        if stop or (max_batches is not None and batches >= max_batches):
            return 1 if stop else 0


def Simulation_BSC_GPU(code, seed, p, SIM, rule=BF_GRADIENT, Num_Frames_OneTime=4096, maxIT=30, exit_mode=EXIT_PER_FRAME, PN_Message=0, pn_seed=0,
                       max_batches=None, leastErrorFrames=50, leastTestFrames=10000, displayStep=40960, dist=None, device=None, log=print):
    """One point of a hard-decision sweep: the binary symmetric channel with crossover probability p, then bit flipping.  A batch is
    PN_CodeWords (PN_Message=1; the all-zero word otherwise) -> BSCChannel_GPU -> LDPC_Decoder_BitFlip_GPU(rule) -> the statistics
    of Simulation_GPU on D, whose flag row is the syndrome.  `seed` (int32[3]) is the RandomModule state, advanced in place by the WHOLE
    batch on every rank, N draws per frame (sharding.bsc_draws_per_frame); the batch loop, its stop rule and the sharding over ranks are
    those of Simulation_GPU.  SIM.SNR is printed as it is: the caller may keep p there."""
    if PN_Message not in (0, 1):
        raise ValueError("PN_Message must be 0 (all-zero codeword) or 1 (random codewords)")
    if rule not in (BF_THRESHOLD, BF_GRADIENT):
        raise ValueError("rule must be BF_THRESHOLD or BF_GRADIENT")
    if exit_mode not in (EXIT_FIXED, EXIT_PER_FRAME):
        raise ValueError("Simulation_BSC_GPU takes EXIT_FIXED or EXIT_PER_FRAME")
    if not (np.isfinite(p) and 0.0 <= p <= 0.5):
        raise ValueError("p must be a crossover probability in [0, 0.5], not %r" % (p,))
    rank = dist.get_rank() if dist is not None and dist.is_initialized() else 0
    world = dist.get_world_size() if dist is not None and dist.is_initialized() else 1
    device = device or torch.device("cuda", torch.cuda.current_device())
    F = Num_Frames_OneTime
    first, count = sharding.shard_frames(F, world, rank)
    per_frame = sharding.bsc_draws_per_frame(code.N)
    dev_cnt = torch.zeros(5, dtype=torch.int64, device=device)
    D = torch.empty((code.N + 1, max(count, 1)), dtype=torch.int32, device=device)
    length = code.K
    batches = 0
    while True:
        SIM.num_Frames += F
        my_seed = sharding.lcg_jump(seed, first * per_frame)
        seed[:] = sharding.lcg_jump(seed, F * per_frame)
        dev_cnt.zero_()
        if count:
            cw = PN_CodeWords(code, pn_seed, count, first_frame=batches * F + first, device=device) if PN_Message else None
            bits = BSCChannel_GPU(my_seed, p, code.N, count, device=device, CodeWord=cw)
            r = LDPC_Decoder_BitFlip_GPU(code, bits, count, rule=rule, max_iter=maxIT, exit_mode=exit_mode, D=D)
            st = torch.cuda.current_stream(device).cuda_stream
            check(lib.bldpc_statistic_per_frame(code._h, _dev_ptr(D), _dev_ptr(cw), count, length, _dev_ptr(r["iters"]), _dev_ptr(dev_cnt), st),
                  "Statistic")
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
            log(format_row(SIM, length))
        if stop or last:
            return 1 if stop else 0


def sweep_bsc(code, ps, seeds=(173, 173, 173), dist=None, log=print, **kw):
    """Simulation_BSC_GPU at every crossover probability of `ps`, seed and counters reset at every point as in `sweep`: a list of
    SimCounters whose SNR field holds p."""
    out = []
    for p in ps:
        SIM = SimCounters()
        SIM.SNR = float(p)
        Simulation_BSC_GPU(code, np.array(seeds, np.int32), float(p), SIM, dist=dist, log=log, **kw)
        out.append(SIM)
    return out


def Simulation_BEC_GPU(code, seed, p, SIM, Num_Frames_OneTime=4096, maxIT=100, PN_Message=0, pn_seed=0, rate_match=None, max_batches=None,
                       leastErrorFrames=50, leastTestFrames=10000, displayStep=40960, dist=None, device=None, log=print, ml=False,
                       ml_max_erased=0, ml_tier="auto"):
    """One point of an erasure sweep: the binary erasure channel with erasure probability p, then peeling, all on packed words.  A batch
    is PN_CodeWords (PN_Message=1; the all-zero word otherwise) -> Hard_Pack_Int, and RM_Select_Bits under a profile -> BECChannel_GPU on
    the N, or the profile's E, transmitted rows -> RM_Recover_Bits under a profile (punctured positions erased, shortened ones known 0)
    -> LDPC_Decoder_Erasure_GPU with Dbits and Ebits only -> Statistic_Bits, where a position still erased is a bit error.  No int32 D
    is made.  `seed` (int32[3]) is the RandomModule state, advanced in place by the WHOLE batch on every rank, one draw per transmitted
    bit (sharding.bec_draws_per_frame); the batch loop, its stop rule and the sharding over ranks are those of Simulation_BSC_GPU.
    rate_match takes linear and circular profiles; under one the bit error rate divides by the prefix bits that are not shortened, as in
    Simulation_GPU.  SIM.SNR is printed as it is: the caller may keep p there.  ml=True: after peeling, LDPC_Decoder_Erasure_ML_GPU on
    peeling's Dbits[:N] and Ebits (frames with more than ml_max_erased erasures left, 0 = M, stay as peeling left them; ml_tier as its
    tier), and the statistics are taken on the new words with peeling's iteration counts."""
    if PN_Message not in (0, 1):
        raise ValueError("PN_Message must be 0 (all-zero codeword) or 1 (random codewords)")
    if not (np.isfinite(p) and 0.0 <= p <= 1.0):
        raise ValueError("p must be an erasure probability in [0, 1], not %r" % (p,))
    if maxIT < 1:
        raise ValueError("maxIT must be at least 1")
    rm = rate_match
    if rm is not None:
        if rm.N != code.N:
            raise ValueError("rate_match is over N=%d positions, the code has N=%d" % (rm.N, code.N))
        if PN_Message and rm.n_short and not np.isin(rm.shorten, code.info_positions).all():
            raise ValueError("rate_match shortens a parity position of the code's generator; only information positions (code.info_positions) "
                             "can be agreed to be 0")
    rank = dist.get_rank() if dist is not None and dist.is_initialized() else 0
    world = dist.get_world_size() if dist is not None and dist.is_initialized() else 1
    device = device or torch.device("cuda", torch.cuda.current_device())
    F = Num_Frames_OneTime
    first, count = sharding.shard_frames(F, world, rank)
    n_tx = rm.E if rm is not None else code.N  # bits per frame that go over the channel
    per_frame = sharding.bec_draws_per_frame(n_tx)
    dev_cnt = torch.zeros(5, dtype=torch.int64, device=device)
    length = code.K
    ber_bits = length - (int((rm.shorten < length).sum()) if rm is not None else 0)  # the prefix bits that carry information
    batches = 0
    while True:
        SIM.num_Frames += F
        my_seed = sharding.lcg_jump(seed, first * per_frame)
        seed[:] = sharding.lcg_jump(seed, F * per_frame)
        dev_cnt.zero_()
        if count:
            cwbits = None
            if PN_Message:
                cwbits = Hard_Pack_Int(PN_CodeWords(code, pn_seed, count, first_frame=batches * F + first, device=device, rate_match=rm))
            tx = RM_Select_Bits(rm, cwbits, count) if (rm is not None and cwbits is not None) else cwbits
            bits, erased = BECChannel_GPU(my_seed, p, n_tx, count, device=device)  # the mask; the channel's words are those of the all-zero word
            if tx is not None:
                bits = tx & ~erased
            if rm is not None:
                bits, erased = RM_Recover_Bits(rm, bits, count, rx_erased=erased)
            r = LDPC_Decoder_Erasure_GPU(code, bits, erased, count, max_iter=maxIT)
            if ml:
                r = dict(LDPC_Decoder_Erasure_ML_GPU(code, r["Dbits"][:code.N], r["Ebits"], count, max_erased=ml_max_erased, tier=ml_tier),
                         iters=r["iters"])
            Statistic_Bits(code, r["Dbits"], count, dev_cnt, Ebits=r["Ebits"], CodeWordBits=cwbits, iters=r["iters"], length=length)
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
            log(" %.4g" % SIM.SNR + format_row(SIM, ber_bits)[len(" %.1f" % SIM.SNR):])  # the row's first column with the digits of a probability
        if stop or last:
            return 1 if stop else 0


def sweep_bec(code, ps, seeds=(173, 173, 173), dist=None, log=print, **kw):
    """Simulation_BEC_GPU at every erasure probability of `ps`, seed and counters reset at every point as in `sweep`: a list of
    SimCounters whose SNR field holds p."""
    out = []
    for p in ps:
        SIM = SimCounters()
        SIM.SNR = float(p)
        Simulation_BEC_GPU(code, np.array(seeds, np.int32), float(p), SIM, dist=dist, log=log, **kw)
        out.append(SIM)
    return out


@dataclass
class HarqCounters:
    """What Simulation_HARQ_GPU accumulates over the batches of one SNR point, all exact integers.  acked[t]: frames acknowledged at
    transmission t (0-based); undetected[t]: those of them whose first K bits differ from the word sent; never_acked: frames still
    unacknowledged after the last transmission; bits_sent: the sum of E_t over the transmissions each frame used.  osd_frames and
    osd_correct (osd=True): the frames reprocessed after the last transmission, and those of them that came out equal to the word sent."""
    num_Frames: int = 0
    acked: list = field(default_factory=list)
    undetected: list = field(default_factory=list)
    never_acked: int = 0
    bits_sent: int = 0
    Total_Iteration: int = 0
    SNR: float = 0.0
    osd_frames: int = field(default=0, repr=False, compare=False)
    osd_correct: int = field(default=0, repr=False, compare=False)

    def ratios(self, info_bits):
        """FER after each transmission (a frame is good once it is acknowledged with the right word), mean transmissions per frame
        and throughput = info_bits * correctly acknowledged frames / bits sent."""
        n, T = max(self.num_Frames, 1), len(self.acked)
        good = np.cumsum([a - u for a, u in zip(self.acked, self.undetected)])
        used = sum((t + 1) * a for t, a in enumerate(self.acked)) + T * self.never_acked
        return dict(FER=[1.0 - g / n for g in good], MeanTx=used / n, Throughput=info_bits * (int(good[-1]) if T else 0) / max(self.bits_sent, 1),
                    AverageIT=self.Total_Iteration / n)


def format_harq_row(SIM, info_bits):
    """SNR NTF, the FER after each transmission, mean transmissions, throughput, iterations per frame."""
    r = SIM.ratios(info_bits)
    return " %.1f %8d  %s  %.3f  %.4f  %.2f" % (SIM.SNR, SIM.num_Frames, " ".join("%6.4e" % x for x in r["FER"]), r["MeanTx"], r["Throughput"],
                                             r["AverageIT"])


def Simulation_HARQ_GPU(code, seed, sigma, SIM, rvs, Num_Frames_OneTime=4096, maxIT=50, exit_mode=EXIT_FIXED, kernel=KERNEL_AUTO,
                        leastErrorFrames=50, leastTestFrames=10000, dist=None, device=None, max_batches=None, log=print, PN_Message=0,
                        pn_seed=0, schedule="flooding", alpha=1.0, stop_rule=None, short_llr=1.0e4, compact=True, keep_D=None, quant=None,
                        n_QAM=2, CONSTELLATION=None, interleave=IL_NONE, fading=None, osd=False, osd_order=0,
                        osd_lambda=0):
    """One SNR point of incremental-redundancy HARQ over BPSK, or over n_QAM-QAM, on the device channel.  rvs = [rm_0, ..., rm_{T-1}]: the profile of
    each transmission (RateMatch.circular or RateMatch, all over code.N with the same shortened positions).  SIM is a HarqCounters.

    A batch: rvs[0] is sent for all F frames (AWGNChannel_RM_GPU: recover semantics) and decoded; row N of D is the ACK.  For
    t = 1 .. T-1, while a frame of this rank is unacknowledged: rvs[t] is combined into the decoder input of the unacknowledged frames
    (AWGNChannel_RM_Combine_GPU under done = D[N]), those frames are gathered (Frames_Gather on torch.nonzero of the flag row), decoded
    and their D and iteration counts scattered back.  compact=False decodes the whole batch instead; the per-frame results of
    EXIT_FIXED and EXIT_PER_FRAME do not depend on the batch, so the counters and D are the same.

    The ACK must hold for the word that was sent.  PN_Message=0 (the all-zero word): the decoder's own flag, flooding (plain, or
    normalised with alpha != 1.0) or layered, EXIT_FIXED or EXIT_PER_FRAME.  PN_Message=1 (random codewords): flooding with EXIT_FIXED
    followed by Syndrome(into_flag_row=True), or layered with STOP_SYNDROME (its default here) and either exit.  EXIT_BATCH_GLOBAL is
    refused: its results depend on the batch.  schedule="bp" (layered sum-product, LDPC_Decoder_BP_GPU) takes what schedule="layered"
    takes, but no `alpha`, and decodes with llr_scale = 2 / sigma^2: the sum of equal-sigma transmissions of a bit is a true LLR under that
    factor.  schedule="quant" (LDPC_Decoder_Quant_GPU with the word lengths of `quant`, a Quant) takes what schedule="layered" takes, but
    no `alpha`: combining stays in fp32 and the decoder quantises the accumulated values with the gain quant.llr_scale.
    A position no transmission has reached yet holds +0.0 and decides 0, so on the all-zero
    word the flag flatters a first transmission with E < Ncb; random codewords do not have that bias.

    Draws: transmission t of a batch owns 2 * E_t * F draws of the noise stream, used or not -- `seed` (int32[3]) is advanced by the
    sum over all T transmissions after every batch on every rank, whatever was acknowledged, and rank r jumps first_r * 2 * E_t draws
    into each.  One all-reduce of the counters per batch.  keep_D (a list) receives this rank's final D of every batch.

    n_QAM != 2 (with CONSTELLATION, host float32 [n_QAM, 2], and PN_Message=1, as for Simulation_GPU): transmission t is RM_Modulate_QAM ->
    AWGNChannel_QAM_GPU -> the bits of RM_Demodulate_QAM_Recover (t = 0) or RM_Demodulate_QAM_Combine under done = D[N], with scale
    1 / (2 sigma^2) and the index rule `interleave` (IL_ROWCOL: the row-column bit interleaver); the receive side runs the fused call or
    Demodulate_QAM -> RM_Recover / RM_Combine, whichever was measured faster (_qam_receive).  It owns 4 * ceil(E_t / m) * F draws, and the channel draws
    for acknowledged frames too: their points are made and never read.  The accumulated values are max-log LLRs already, so
    schedule="bp" decodes with llr_scale = 1.0.  The caller passes the sigma of that n_QAM (nbldpc.sigma_of; sweep_harq does).

    fading (a Fading): every transmission sees a fading realisation of its own.  Transmission t draws the gains of its S_t channel uses
    (E_t over BPSK, ceil(E_t / m) over QAM) for all F frames of the batch from the fading stream, fading.seed -- ceil(S_t / Lc) draws
    per frame, owned whether a frame is acknowledged or not, so the stream's position after a batch depends on nothing that happened in
    it -- and runs as the composition RM_Select (or RM_Modulate_QAM) -> the fading channel -> (Demodulate_QAM_Fading ->) RM_Recover
    for t = 0, RM_Combine under done = D[N] after it.  The noise stream is used exactly as without fading.

    osd=True (schedule 'layered', 'bp' or 'quant' with stop_rule=STOP_SYNDROME; refused elsewhere): after the last transmission of a batch
    the frames still unacknowledged are reprocessed by LDPC_Decoder_OSD_GPU on the D and app of their last decode, in place, so keep_D
    receives codewords with flag 1 in their columns.  A reprocessed frame is NOT acknowledged by that: reprocessing always returns a
    codeword, so its flag says nothing about the word sent.  The acknowledgement stays the decoder's flag, and acked, undetected,
    never_acked, bits_sent and the iterations are what they are with osd=False; SIM.osd_frames and SIM.osd_correct count the frames
    reprocessed and those of them that came out equal to the word sent, and the log row ends with both.  osd_order and osd_lambda are
    those of Simulation_GPU."""
    if PN_Message not in (0, 1):
        raise ValueError("PN_Message must be 0 (all-zero codeword) or 1 (random codewords)")
    bp, layered = _check_schedule(schedule, alpha, quant)
    if schedule == "hard":
        raise ValueError("HARQ takes no schedule='hard': soft combining has no meaning for hard decisions, and an unsent position is an erasure")
    if exit_mode not in (EXIT_FIXED, EXIT_PER_FRAME):
        raise ValueError("HARQ takes EXIT_FIXED or EXIT_PER_FRAME: the results of EXIT_BATCH_GLOBAL depend on the batch")
    if not layered and stop_rule is not None:
        raise ValueError("stop_rule belongs to schedule='layered', schedule='bp' and schedule='quant'")
    norm = not layered and alpha != 1.0
    if layered:
        if stop_rule is None:
            stop_rule = STOP_SYNDROME if PN_Message else STOP_PREFIX
        if stop_rule not in (STOP_PREFIX, STOP_SYNDROME):
            raise ValueError("stop_rule must be STOP_PREFIX or STOP_SYNDROME")
        if PN_Message == 1 and stop_rule != STOP_SYNDROME and exit_mode != EXIT_FIXED:
            raise ValueError("PN_Message=1 with per-frame exit needs stop_rule=STOP_SYNDROME: STOP_PREFIX tests for the all-zero word")
    elif PN_Message == 1 and exit_mode != EXIT_FIXED:
        raise ValueError("PN_Message=1 needs exit_mode=EXIT_FIXED: the flooding decoders' early exit tests for the all-zero word")
    _check_osd(osd, schedule, stop_rule, osd_order, osd_lambda)
    qam_m, con = _check_qam(n_QAM, CONSTELLATION, PN_Message, interleave)
    _check_fading(fading, True, exit_mode)
    rvs = list(rvs) if rvs is not None else []
    if not rvs:
        raise ValueError("rvs must hold at least one profile")
    for t, rm in enumerate(rvs):
        if rm.N != code.N:
            raise ValueError("rvs[%d] is over N=%d positions, the code has N=%d" % (t, rm.N, code.N))
        if not np.array_equal(rm.shorten, rvs[0].shorten):
            raise ValueError("rvs[%d] shortens other positions than rvs[0]: the shortened bits are fixed by the codeword, not by the transmission" % t)
    if not (np.isfinite(short_llr) and short_llr > 0):
        raise ValueError("short_llr must be finite and > 0, not %r" % (short_llr,))
    if PN_Message and rvs[0].n_short and not np.isin(rvs[0].shorten, code.info_positions).all():
        raise ValueError("rvs shorten a parity position of the code's generator; only information positions (code.info_positions) "
                         "can be agreed to be 0")
    T = len(rvs)
    if not SIM.acked:
        SIM.acked, SIM.undetected = [0] * T, [0] * T
    if len(SIM.acked) != T:
        raise ValueError("SIM holds counters of %d transmissions, rvs has %d" % (len(SIM.acked), T))
    rank = dist.get_rank() if dist is not None and dist.is_initialized() else 0
    world = dist.get_world_size() if dist is not None and dist.is_initialized() else 1
    device = device or torch.device("cuda", torch.cuda.current_device())
    F = Num_Frames_OneTime
    first, count = sharding.shard_frames(F, world, rank)
    N, K = code.N, code.K
    info_bits = K - rvs[0].n_short
    cnt = torch.zeros(2 * T + 3, dtype=torch.int64, device=device)  # acked[T], undetected[T], never, bits, iterations
    osd_cnt = torch.zeros(2, dtype=torch.int64, device=device) if osd else None
    last_app = [None]  # osd: the app of the latest decode()
    con_dev = torch.from_numpy(con).to(device) if qam_m else None
    llr_scale = 1.0 if qam_m else 2.0 / (sigma * sigma)  # schedule="bp": what makes the accumulated values true LLRs
    qam_scale = 1.0 / (2.0 * sigma * sigma)

    def decode(y, D):
        """Decode y into D, leave the ACK in row N, return the iterations of every frame (int32 [F'])."""
        if layered:
            if bp:
                r = LDPC_Decoder_BP_GPU(code, y, max_iter=maxIT, llr_scale=llr_scale, length=K, exit_mode=exit_mode, stop_rule=stop_rule, D=D,
                                        want_app=osd)
            elif quant is not None:
                r = LDPC_Decoder_Quant_GPU(code, y, quant, max_iter=maxIT, length=K, exit_mode=exit_mode, stop_rule=stop_rule, D=D, want_app=osd)
            else:
                r = LDPC_Decoder_Layered_GPU(code, y, max_iter=maxIT, alpha=alpha, length=K, exit_mode=exit_mode, stop_rule=stop_rule, D=D,
                                             want_app=osd)
            if PN_Message and stop_rule != STOP_SYNDROME:
                Syndrome(code, D, into_flag_row=True)
            last_app[0] = r["app"]
            return r["iters"]
        r = LDPC_Decoder_GPU(code, y, max_iter=maxIT, length=K, exit_mode=exit_mode, kernel=kernel, D=D, alpha=alpha if norm else None)
        if PN_Message:
            Syndrome(code, D, into_flag_row=True)
        if r.get("iters") is not None:
            return r["iters"]
        return torch.full((y.shape[1],), r["iteraTime"], dtype=torch.int32, device=device)

    batches = 0
    while True:
        SIM.num_Frames += F
        cnt.zero_()
        if osd:
            osd_cnt.zero_()
        if count:
            cw = PN_CodeWords(code, pn_seed, count, first_frame=batches * F + first, device=device, rate_match=rvs[0]) if PN_Message else None
            D = torch.empty((N + 1, count), dtype=torch.int32, device=device)
            acked = torch.zeros(count, dtype=torch.bool, device=device)
        for t, rm in enumerate(rvs):
            per_frame = sharding.qam_draws_per_frame(rm.E, qam_m) if qam_m else sharding.binary_draws_per_frame(rm.E)
            my_seed = sharding.lcg_jump(seed, first * per_frame)
            seed[:] = sharding.lcg_jump(seed, F * per_frame)  # owned by this transmission whether it is used or not
            skip = not count or (t and bool(acked.all()))
            if fading is not None:  # and so are its gains: the fading seed moves before anything can skip the transmission
                gain = _fading_gains(fading, sharding.fading_uses(rm.E, qam_m), F, first, 0 if skip else count, device)
            if skip:
                continue
            active = ~acked
            if fading is not None:
                llr = _fading_transmit(gain, my_seed, sigma, cw, rm.E, count, qam_m, con_dev, interleave, rm)
            elif qam_m:  # the points of every frame, acknowledged or not: the QAM channel has no done mask
                rx = AWGNChannel_QAM_GPU(my_seed, sigma, RM_Modulate_QAM(rm, cw, qam_m, interleave=interleave), con_dev)
            if t == 0:
                if fading is not None:
                    acc = RM_Recover(rm, llr, short_llr)
                elif qam_m:
                    acc = _qam_receive(rm, rx, con_dev, qam_scale, short_llr, interleave)
                else:
                    acc = AWGNChannel_RM_GPU(rm, my_seed, sigma, count, device=device, CodeWord=cw, short_llr=short_llr)
                iters = decode(acc, D)
                app = last_app[0]
            else:
                if fading is not None:
                    RM_Combine(rm, llr, acc, done=D[N], short_llr=short_llr)
                elif qam_m:
                    _qam_receive(rm, rx, con_dev, qam_scale, short_llr, interleave, acc=acc, done=D[N])
                else:
                    AWGNChannel_RM_Combine_GPU(rm, my_seed, sigma, acc, done=D[N], CodeWord=cw, short_llr=short_llr)
                if compact:
                    idx = torch.nonzero(active).view(-1).to(torch.int32)
                    Da = torch.empty((N + 1, idx.numel()), dtype=torch.int32, device=device)
                    ia = decode(Frames_Gather(acc, idx), Da)
                    Frames_Scatter(Da, idx, D)
                    Frames_Scatter(ia, idx, iters)
                    if osd:
                        Frames_Scatter(last_app[0], idx, app)
                else:
                    iters = decode(acc, D)
                    app = last_app[0]
            now = (D[N] != 0) & active
            wrong = ((D[:K] != cw[:K]) if cw is not None else (D[:K] != 0)).any(0)
            cnt[t] += now.sum()
            cnt[T + t] += (now & wrong).sum()
            cnt[2 * T + 1] += rm.E * active.sum()
            cnt[2 * T + 2] += iters[active].sum()
            acked |= now
        if count:
            cnt[2 * T] += (~acked).sum()
            if osd:  # the flag row has served as the acknowledgement: from here on it says "codeword"
                _osd_reprocess(code, D, app, cw, osd_cnt, osd_order, osd_lambda)
            if keep_D is not None:
                keep_D.append(D)
        sharding.allreduce_counters(cnt, dist)
        c = cnt.cpu().tolist()
        for t in range(T):
            SIM.acked[t] += c[t]
            SIM.undetected[t] += c[T + t]
        SIM.never_acked += c[2 * T]
        SIM.bits_sent += c[2 * T + 1]
        SIM.Total_Iteration += c[2 * T + 2]
        if osd:
            o = sharding.allreduce_counters(osd_cnt, dist).cpu().tolist()
            SIM.osd_frames += o[0]
            SIM.osd_correct += o[1]
        batches += 1
        errors = SIM.never_acked + sum(SIM.undetected)
        stop = errors >= leastErrorFrames and SIM.num_Frames >= leastTestFrames
        last = max_batches is not None and batches >= max_batches
        if rank == 0 and log and (stop or last):
            log(format_harq_row(SIM, info_bits) + ("  OSD %d %d" % (SIM.osd_frames, SIM.osd_correct) if osd else ""))
        if stop or last:
            return 1 if stop else 0


def sweep_harq(code, rvs, startSNR=0.0, stopSNR=13.0, stepSNR=0.2, snrtype=1, seeds=(173, 173, 173), dist=None, log=print, n_QAM=2, **kw):
    """The sweep of `sweep` over Simulation_HARQ_GPU: a list of HarqCounters, one per SNR point.  Under Eb/N0 (snrtype 0) sigma comes
    from the rate of the FIRST transmission, rvs[0].rate(code.K): the operating point is named by what is sent when nothing goes wrong,
    and the later transmissions run over the same channel.  With n_QAM != 2 (pass the constellation itself as CONSTELLATION=...) sigma
    is the GF(q) program's at that rate, nbldpc_sigma(SNR, snrtype, n_QAM, rate), as in `sweep`."""
    out = []
    rate = rvs[0].rate(code.K)
    if n_QAM != 2:
        kw["n_QAM"] = n_QAM
    fading_seed0 = kw["fading"].seed.tolist() if kw.get("fading") is not None else None
    for snr in snr_grid(startSNR, stopSNR, stepSNR):
        seed = np.array(seeds, np.int32)
        if fading_seed0 is not None:  # the fading stream restarts at every point, as the noise stream does
            kw["fading"] = Fading(kw["fading"].Lc, fading_seed0)
        SIM = HarqCounters()
        SIM.SNR = snr
        sigma = nb_sigma_of(snr, rate, snrtype, n_QAM) if n_QAM != 2 else sigma_of(snr, snrtype, rate)
        Simulation_HARQ_GPU(code, seed, sigma, SIM, rvs, dist=dist, log=log, **kw)
        out.append(SIM)
    return out


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
    fading_seed0 = kw["fading"].seed.tolist() if kw.get("fading") is not None else None
    for snr in snr_grid(startSNR, stopSNR, stepSNR):
        seed = np.array(seeds, np.int32)  # reset at every point (main.cu:117-119)
        if fading_seed0 is not None:  # and so is the fading stream
            kw["fading"] = Fading(kw["fading"].Lc, fading_seed0)
        SIM = SimCounters()
        SIM.SNR = snr
        sigma = nb_sigma_of(snr, rate, snrtype, n_QAM) if n_QAM != 2 else sigma_of(snr, snrtype, rate)
        Simulation_GPU(code, seed, sigma, SIM, dist=dist, log=log, **kw)
        out.append(SIM)
    return out
