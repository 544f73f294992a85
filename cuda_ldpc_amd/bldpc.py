"""Host-side mirror of the reference's binary LDPC entry points.

Same names and argument meaning as bldpc_实习/{Simulation,LDPC_Decoder}.cu; the
compile-time macros of define.cuh (J, L, Z, Num_Frames_OneTime, maxIT, msgLen)
become run-time arguments.  Everything computes through the C ABI of
include/bldpc.h on the GPU; tensors are torch CUDA(HIP) tensors.
"""
import collections
import ctypes
from dataclasses import dataclass, field

import numpy as np
import torch

from ._lib import LdpcError, bldpc_quant, check, lib
from .nbldpc import Get_CONSTELLATION  # noqa: F401  -- the constellation files serve both code families

EXIT_FIXED, EXIT_BATCH_GLOBAL, EXIT_PER_FRAME = 0, 1, 2
KERNEL_AUTO, KERNEL_TABLE, KERNEL_QC_LDS = 0, 1, 2
STOP_PREFIX, STOP_SYNDROME = 0, 1  # stop rules of the layered decoder (bldpc.h)
BF_THRESHOLD, BF_GRADIENT = 0, 1  # rules of the bit-flipping decoder (bldpc.h)
BITFLIP_LDS_BOUND = 160 * 1024 - 1024  # the dynamic LDS a workgroup of k_bf may ask for: a code fits when its plan's figure is within it
IL_NONE, IL_ROWCOL = 0, 1  # index rules of the QAM modem (bldpc.h): bit b of symbol s is bit s*m + b, or b*Ns + s (row-column interleaver)


def _np_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _dev_ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _check_D(D, N, F, dev):
    """A caller-supplied D goes to the C ABI as a raw pointer: a wrong shape is an out-of-bounds device write and a
    misaligned one faults in the 16-byte stores of the unpack kernel -- refuse both here."""
    if not (torch.is_tensor(D) and D.is_cuda and D.device == dev and D.dtype == torch.int32 and D.is_contiguous()
            and D.dim() == 2 and tuple(D.shape) == (N + 1, F)):
        raise ValueError("D must be a contiguous CUDA int32 tensor [N+1=%d, F=%d] on %s" % (N + 1, F, dev))
    if D.data_ptr() % 16:
        raise ValueError("D must be 16-byte aligned")


def _check_counters(counters, n, dev):
    if not (torch.is_tensor(counters) and counters.is_cuda and counters.device == dev and counters.dtype == torch.int64
            and counters.is_contiguous() and counters.numel() >= n):
        raise ValueError("counters must be a contiguous CUDA int64 tensor of at least %d elements on %s" % (n, dev))


def Get_H(path, J, L):
    """Get_H (Simulation.cu:292-354): -> (H[J*L], Weight_Checknode[J+1], Weight_Variablenode[L+1]) int32 host arrays."""
    H = np.zeros(J * L, np.int32)
    wc = np.zeros(J + 1, np.int32)
    wv = np.zeros(L + 1, np.int32)
    check(lib.bldpc_read_blockh(str(path).encode(), J, L, _np_ptr(H), _np_ptr(wc), _np_ptr(wv)), "Get_H")
    return H, wc, wv


def Transform_H(H, J, L, Z, Weight_Checknode, Weight_Variablenode, as_written=False):
    """Transform_H (Simulation.cu:363-387): -> Address_Variablenode[N*Wv] int32 (host)."""
    H = np.ascontiguousarray(H, np.int32)
    wc = np.ascontiguousarray(Weight_Checknode, np.int32)
    wv = np.ascontiguousarray(Weight_Variablenode, np.int32)
    addr = np.zeros(L * Z * int(wv[L]), np.int32)
    check(lib.bldpc_transform_h(_np_ptr(H), J, L, Z, _np_ptr(wc), _np_ptr(wv), _np_ptr(addr), 1 if as_written else 0),
          "Transform_H")
    return addr


def AWGNChannel_CPU(seed, sigma, N, F, CodeWord=None):
    """AWGNChannel_CPU (LDPC_Encoder.cu:25-43). seed: int32[3] numpy array, advanced in place (AWGN->seed).
    Returns Channel_Out as a host float32 array [N, F] (frame-fastest)."""
    if not (isinstance(seed, np.ndarray) and seed.dtype == np.int32 and seed.size == 3):
        raise ValueError("seed must be an int32 numpy array of 3")
    out = np.empty((N, F), np.float32)
    cw = None if CodeWord is None else np.ascontiguousarray(CodeWord, np.int32)
    check(lib.bldpc_awgn_channel_host(_np_ptr(seed), ctypes.c_float(sigma), _np_ptr(out), None if cw is None else _np_ptr(cw), N, F),
          "AWGNChannel_CPU")
    return out


def AWGNChannel_GPU(seed, sigma, N, F, device=None, CodeWord=None, stream=None):
    """The same channel generated on the device (bldpc_awgn_channel_device): identical RandomModule draws via LCG
    jump-ahead, device libm for the Box-Muller transform.  Returns a CUDA float32 tensor [N, F]; seed advanced."""
    if not (isinstance(seed, np.ndarray) and seed.dtype == np.int32 and seed.size == 3):
        raise ValueError("seed must be an int32 numpy array of 3")
    device = device or torch.device("cuda", torch.cuda.current_device())
    out = torch.empty((N, F), dtype=torch.float32, device=device)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(device)).cuda_stream)
    check(lib.bldpc_awgn_channel_device(_np_ptr(seed), ctypes.c_float(sigma), _dev_ptr(out), _dev_ptr(CodeWord), N, F, st), "AWGNChannel_GPU")
    return out


def sigma_of(SNR, snrtype=1, rate=0.0):
    """sigma of a sweep point (main.cu:120-127); snrtype 1 = Es/N0 (the reference default, define.cuh:45)."""
    return float(lib.bldpc_sigma(np.float32(SNR), snrtype, np.float32(rate)))


_QC_VARIANT_FIELDS = ("NF", "J", "L", "Z", "WC", "WV", "G", "MINW", "CPT", "regstate", "loc", "has_pf", "U", "threads", "lds_bytes")


def qc_variants():
    """The table of ahead-of-time fused kernel variants (bldpc_qc_variant_info), in selection order: a list of dicts with the
    fields of include/bldpc.h plus index and tag.  CPT holds NG for the "regstate-halo" entries.  Host only, no device needed."""
    out = []
    for i in range(int(lib.bldpc_qc_variant_count())):
        d = np.zeros(16, np.int32)
        tag = ctypes.c_char_p()
        check(lib.bldpc_qc_variant_info(i, _np_ptr(d), ctypes.byref(tag)), "bldpc_qc_variant_info")
        v = dict(zip(_QC_VARIANT_FIELDS, (int(x) for x in d)))
        v.update(index=i, tag=tag.value.decode(), has_pf=bool(v["has_pf"]))
        out.append(v)
    return out


QcPlanHost = collections.namedtuple("QcPlanHost", "variant variant_per_frame lds_bytes lc WVS frames_per_wg info digest")


def qc_plan_host(H, Z, pin=-1, no_local=False, no_halo=False, local_per_frame=False):
    """bldpc_qc_plan_host: the fused-kernel plan a code object of the block matrix H [J, L] would get (pin, no_local, no_halo,
    local_per_frame: as BLDPC_QC_VARIANT, BLDPC_NO_LOCAL, BLDPC_NO_HALO, BLDPC_LOCAL_PER_FRAME), with the FNV-1a digests of its
    tables.  Host only, no device needed.  info: int32 [8], digest: uint64 [8] as in include/bldpc.h."""
    H = np.ascontiguousarray(H, np.int32)
    J, L = H.shape
    info, digest = np.zeros(8, np.int32), np.zeros(8, np.uint64)
    flags = (1 if no_local else 0) | (2 if no_halo else 0) | (4 if local_per_frame else 0)
    check(lib.bldpc_qc_plan_host(J, L, int(Z), _np_ptr(H), int(pin), flags, _np_ptr(info), _np_ptr(digest)), "bldpc_qc_plan_host")
    return QcPlanHost(*(int(x) for x in info[:6]), info, digest)


class BinaryCode:
    """Device-resident code object (bldpc_code).  Build with from_blockh / from_shifts / from_table."""

    def __init__(self, handle, J, L, Z):
        self._h = handle
        self.J, self.L, self.Z = J, L, Z
        d = np.zeros(8, np.int32)
        check(lib.bldpc_code_dims(self._h, _np_ptr(d)), "bldpc_code_dims")
        self.N, self.M, self.K, self.Wc, self.Wv, self.nnz, self.levels, self.frames_per_wg = (int(x) for x in d)

    @classmethod
    def from_shifts(cls, H, J, L, Z):
        H = np.ascontiguousarray(H, np.int32)
        if H.size != J * L:
            raise ValueError("H must hold J*L shifts")
        h = ctypes.c_void_p()
        check(lib.bldpc_code_create_qc(J, L, Z, _np_ptr(H), ctypes.byref(h)), "bldpc_code_create_qc")
        return cls(h, J, L, Z)

    @classmethod
    def from_blockh(cls, path, J, L, Z):
        H, _, _ = Get_H(path, J, L)
        return cls.from_shifts(H, J, L, Z)

    @classmethod
    def from_table(cls, J, L, Z, Weight_Checknode, Weight_Variablenode, Address_Variablenode):
        wc = np.ascontiguousarray(Weight_Checknode, np.int32)
        wv = np.ascontiguousarray(Weight_Variablenode, np.int32)
        addr = np.ascontiguousarray(Address_Variablenode, np.int32)
        if wc.size != J + 1 or wv.size != L + 1 or addr.size != L * Z * int(wv[L]):
            raise ValueError("table shapes do not match J, L, Z")
        h = ctypes.c_void_p()
        check(lib.bldpc_code_create_table(J, L, Z, _np_ptr(wc), _np_ptr(wv), _np_ptr(addr), ctypes.byref(h)),
              "bldpc_code_create_table")
        return cls(h, J, L, Z)

    def _encoder_info(self):
        if getattr(self, "_info_pos", None) is None:
            k, r = ctypes.c_int(0), ctypes.c_int(0)
            check(lib.bldpc_encoder_info(self._h, ctypes.byref(k), ctypes.byref(r), None), "bldpc_encoder_info")
            pos = np.zeros(k.value, np.int32)
            check(lib.bldpc_encoder_info(self._h, ctypes.byref(k), ctypes.byref(r), _np_ptr(pos)), "bldpc_encoder_info")
            self._K_info, self._rank, self._info_pos = k.value, r.value, pos
        return self._K_info, self._rank, self._info_pos

    @property
    def K_info(self):
        """K' = N - rank(H): information bits per codeword of the systematic encoder (builds the generator on first use)."""
        return self._encoder_info()[0]

    @property
    def rank(self):
        return self._encoder_info()[1]

    @property
    def info_positions(self):
        """int32 [K'] (host, ascending): codeword position of each information bit."""
        return self._encoder_info()[2]

    @property
    def last_kernel(self):
        return lib.bldpc_last_kernel(self._h).decode()

    def qc_info(self):
        """bldpc_code_qc_info: dict(variant, variant_per_frame, persist_grid, frames_per_wg, force_regroup, no_persist,
        persist_grid_per_frame) of the fused-kernel plan; the variant indices are -1 where there is no such plan."""
        d = np.zeros(8, np.int32)
        check(lib.bldpc_code_qc_info(self._h, _np_ptr(d)), "bldpc_code_qc_info")
        return dict(variant=int(d[0]), variant_per_frame=int(d[1]), persist_grid=int(d[2]), frames_per_wg=int(d[3]),
                    force_regroup=bool(d[4]), no_persist=bool(d[5]), persist_grid_per_frame=int(d[6]))

    def bitflip_info(self):
        """bldpc_bitflip_info: dict(lds_bytes, threads, frames_per_wg, fits) of the bit-flipping kernel k_bf for this code, without a launch."""
        d = np.zeros(4, np.int32)
        check(lib.bldpc_bitflip_info(self._h, _np_ptr(d)), "bldpc_bitflip_info")
        return dict(lds_bytes=int(d[0]), threads=int(d[1]), frames_per_wg=int(d[2]), fits=int(d[0]) <= BITFLIP_LDS_BOUND)

    def erasure_info(self):
        """bldpc_erasure_info: dict(lds_bytes, threads, frames_per_wg, fits) of the peeling kernel k_er for this code, without a launch."""
        d = np.zeros(4, np.int32)
        check(lib.bldpc_erasure_info(self._h, _np_ptr(d)), "bldpc_erasure_info")
        return dict(lds_bytes=int(d[0]), threads=int(d[1]), frames_per_wg=int(d[2]), fits=int(d[0]) <= ERASURE_LDS_BOUND)

    def osd_info(self, tier="auto", order=0):
        """bldpc_osd_info: dict(lds_bytes, threads, tier, slots) of the reprocessing kernel k_osd for this code, without a launch; slots
        is the workspace tier's at F = 65536.  Builds the code's generator on first use, for the rank of H.  order >= 1: bldpc_osd_w_info,
        the same of k_osd_w at that order."""
        d = np.zeros(4, np.int32)
        if order:
            check(lib.bldpc_osd_w_info(self._h, _ml_tier(tier), int(order), _np_ptr(d)), "bldpc_osd_w_info")
        else:
            check(lib.bldpc_osd_info(self._h, _ml_tier(tier), _np_ptr(d)), "bldpc_osd_info")
        return _osd_info(d)

    def erasure_ml_info(self, max_erased=0, tier="auto"):
        """bldpc_erasure_ml_info: dict(matrix_bytes, threads, tier, slots) of the elimination kernel k_er_ml for this code at max_erased
        (0: M), without a launch; slots is the workspace tier's at F = 65536."""
        d = np.zeros(4, np.int32)
        check(lib.bldpc_erasure_ml_info(self._h, int(max_erased), _ml_tier(tier), _np_ptr(d)), "bldpc_erasure_ml_info")
        return _ml_info(d)

    @property
    def qc_variant(self):
        """Index into qc_variants() of the fused kernel variant this code runs on (-1: the table kernels serve it)."""
        return self.qc_info()["variant"]

    @property
    def qc_variant_per_frame(self):
        """Index of the nested plan that serves the per-frame passes (-1: the plan of qc_variant serves them itself)."""
        return self.qc_info()["variant_per_frame"]

    @property
    def persist_grid(self):
        """Workgroups of the persistent per-frame kernel of the plan that serves the per-frame passes (0: it has none)."""
        q = self.qc_info()
        return q["persist_grid_per_frame"] if q["variant_per_frame"] >= 0 else q["persist_grid"]

    def set_profiling(self, enable=True):
        check(lib.bldpc_set_profiling(self._h, 1 if enable else 0), "bldpc_set_profiling")

    def last_kernel_ms(self):
        """Elapsed ms of the dominant kernel of the last LDPC_Decoder_GPU call (HIP events on its stream)."""
        ms = ctypes.c_float(0)
        check(lib.bldpc_last_kernel_ms(self._h, ctypes.byref(ms)), "bldpc_last_kernel_ms")
        return ms.value

    def kernel_ms_mean(self):
        """(mean ms of the dominant kernel, calls averaged) over the profiled decode calls since the last query -- every call
        records its own event pair, nothing synchronises in between (bldpc_kernel_ms_mean)."""
        ms, n = ctypes.c_float(0), ctypes.c_int(0)
        check(lib.bldpc_kernel_ms_mean(self._h, ctypes.byref(ms), ctypes.byref(n)), "bldpc_kernel_ms_mean")
        return ms.value, n.value

    def close(self):
        if self._h:
            lib.bldpc_code_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def generator_host(H, J, L, Z):
    """bldpc_generator_host: the systematic generator of the QC code with block shifts H, on the host (no device).
    Returns dict(K_info, rank, info_pos=int32 [K'], P=uint64 [rank, ceil(K'/64)]): parity bit r (r-th non-information
    position, ascending) = XOR of the information bits j with bit j%64 of P[r, j//64] set."""
    H = np.ascontiguousarray(H, np.int32)
    if H.size != J * L:
        raise ValueError("H must hold J*L shifts")
    k, r = ctypes.c_int(0), ctypes.c_int(0)
    check(lib.bldpc_generator_host(J, L, Z, _np_ptr(H), ctypes.byref(k), ctypes.byref(r), None, None), "bldpc_generator_host")
    pos = np.zeros(k.value, np.int32)
    P = np.zeros((r.value, (k.value + 63) // 64), np.uint64)
    check(lib.bldpc_generator_host(J, L, Z, _np_ptr(H), ctypes.byref(k), ctypes.byref(r), _np_ptr(pos), _np_ptr(P)), "bldpc_generator_host")
    return dict(K_info=k.value, rank=r.value, info_pos=pos, P=P)


def _check_cw(CodeWord, N, F, dev):
    if not (torch.is_tensor(CodeWord) and CodeWord.is_cuda and CodeWord.device == dev and CodeWord.dtype == torch.int32
            and CodeWord.is_contiguous() and tuple(CodeWord.shape) == (N, F)):
        raise ValueError("CodeWord must be a contiguous CUDA int32 tensor [N=%d, F=%d] on %s" % (N, F, dev))


def Encode(code, msg, CodeWord=None, stream=None):
    """bldpc_encode: msg = CUDA int32 tensor [K', F] (frame-fastest, bit 0 read) -> CodeWord int32 [N, F] on the device,
    systematic on code.info_positions."""
    K = code.K_info
    if not (torch.is_tensor(msg) and msg.is_cuda and msg.dtype == torch.int32 and msg.is_contiguous() and msg.dim() == 2
            and msg.shape[0] == K and msg.shape[1] > 0):
        raise ValueError("msg must be a contiguous CUDA int32 tensor [K'=%d, F]" % K)
    F, dev = int(msg.shape[1]), msg.device
    if CodeWord is None:
        CodeWord = torch.empty((code.N, F), dtype=torch.int32, device=dev)
    else:
        _check_cw(CodeWord, code.N, F, dev)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)
    check(lib.bldpc_encode(code._h, _dev_ptr(msg), F, _dev_ptr(CodeWord), st), "Encode")
    return CodeWord


def PN_CodeWords(code, seed, F, first_frame=0, want_msg=False, device=None, CodeWord=None, stream=None, rate_match=None):
    """bldpc_encode_random: the codewords of frames first_frame .. first_frame+F-1 of the message stream `seed`
    (counter-based rule of bldpc.h, mirrored by pn_messages below).  Returns CodeWord int32 [N, F] on the device, or
    (CodeWord, msg [K', F]) with want_msg.  rate_match (a RateMatch over the code's N): bldpc_rm_encode_random, every message bit on
    a shortened position forced to 0; a shortened position outside code.info_positions is refused."""
    if F <= 0 or first_frame < 0:
        raise ValueError("F must be positive and first_frame >= 0")
    if rate_match is not None and rate_match.N != code.N:
        raise ValueError("rate_match is over N=%d positions, the code has N=%d" % (rate_match.N, code.N))
    device = device or torch.device("cuda", torch.cuda.current_device())
    if CodeWord is None:
        CodeWord = torch.empty((code.N, F), dtype=torch.int32, device=device)
    else:
        _check_cw(CodeWord, code.N, F, device)
    msg = torch.empty((code.K_info, F), dtype=torch.int32, device=device) if want_msg else None
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(device)).cuda_stream)
    if rate_match is not None:
        check(lib.bldpc_rm_encode_random(code._h, rate_match._h, ctypes.c_ulonglong(int(seed) % (1 << 64)), int(first_frame), F, _dev_ptr(msg),
                                         _dev_ptr(CodeWord), st), "PN_CodeWords")
    else:
        check(lib.bldpc_encode_random(code._h, ctypes.c_ulonglong(int(seed) % (1 << 64)), int(first_frame), F, _dev_ptr(msg), _dev_ptr(CodeWord), st),
              "PN_CodeWords")
    return (CodeWord, msg) if want_msg else CodeWord


_M64 = (1 << 64) - 1


def splitmix64(x):
    """The first output of SplitMix64 seeded with x (uint64 numpy array or int), as bldpc.h defines it."""
    with np.errstate(over="ignore"):
        z = np.asarray(x, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def pn_messages(seed, K_info, F, first_frame=0):
    """Host mirror of bldpc_encode_random's message rule: int32 [K', F] (frame-fastest)."""
    KW = (K_info + 63) // 64
    g = np.arange(first_frame, first_frame + F, dtype=np.uint64)
    with np.errstate(over="ignore"):
        ctr = np.uint64(int(seed) & _M64) + g[None, :] * np.uint64(KW) + np.arange(KW, dtype=np.uint64)[:, None]
    words = splitmix64(ctr)  # [KW, F]
    k = np.arange(K_info)
    return ((words[k // 64] >> (k % 64).astype(np.uint64)[:, None]) & np.uint64(1)).astype(np.int32)


def Syndrome(code, D, into_flag_row=True, stream=None):
    """bldpc_syndrome: H * d_f == 0 for every frame of the hard bits D (CUDA int32 [N+1, F], or [N, F] with
    into_flag_row=False).  into_flag_row writes the flag into row N of D, where Statistic reads it.
    Returns dict(flag=int32 [F], unsat=int32 [F]: unsatisfied checks) on the device."""
    if not (torch.is_tensor(D) and D.is_cuda and D.dtype == torch.int32 and D.is_contiguous() and D.dim() == 2):
        raise ValueError("D must be a contiguous CUDA int32 tensor")
    rows = code.N + 1 if into_flag_row else None
    if (rows is not None and D.shape[0] != rows) or D.shape[0] < code.N or D.shape[1] <= 0:
        raise ValueError("D must be [N+1=%d, F]%s" % (code.N + 1, "" if into_flag_row else " or [N, F]"))
    F, dev = int(D.shape[1]), D.device
    flag = D[code.N] if into_flag_row else torch.empty(F, dtype=torch.int32, device=dev)
    unsat = torch.empty(F, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)
    check(lib.bldpc_syndrome(code._h, _dev_ptr(D), F, _dev_ptr(flag), _dev_ptr(unsat), st), "Syndrome")
    return dict(flag=flag, unsat=unsat)


def LDPC_Decoder_GPU(code, Channel_Out, max_iter=50, length=0, exit_mode=EXIT_BATCH_GLOBAL, kernel=KERNEL_AUTO,
                     D=None, want_app=False, want_flag_hist=False, stream=None, alpha=None):
    """LDPC_Decoder_GPU (LDPC_Decoder.cu:23-164).

    Channel_Out: CUDA float32 tensor [N, F] (frame-fastest, as the reference).
    Returns dict(D=int32 [N+1, F] on device, iteraTime=int, app=[N, F] or None, flag_hist=uint64-as-int64 [F] or None).

    exit_mode=EXIT_PER_FRAME (bldpc_decode_per_frame): every frame stops on its own flag, as the reference does with a
    batch of one frame; the result then carries iters=int32 [F] on the device (iterations per frame) and iteraTime is None.

    alpha=None is the reference's un-normalised min-sum.  A number in (0, 1] runs the normalised kernels (bldpc_decode_normalised:
    every check message times alpha, 1.0 included): EXIT_FIXED (iteraTime = max_iter) or EXIT_PER_FRAME, no flag history.
    """
    if not (Channel_Out.is_cuda and Channel_Out.dtype == torch.float32 and Channel_Out.is_contiguous()):
        raise ValueError("Channel_Out must be a contiguous CUDA float32 tensor")
    if Channel_Out.dim() != 2 or Channel_Out.shape[0] != code.N:
        raise ValueError("Channel_Out must be [N=%d, F]" % code.N)
    F = int(Channel_Out.shape[1])
    dev = Channel_Out.device
    if D is None:
        D = torch.empty((code.N + 1, F), dtype=torch.int32, device=dev)
    else:
        _check_D(D, code.N, F, dev)
    if alpha is not None and (exit_mode == EXIT_BATCH_GLOBAL or want_flag_hist):
        raise ValueError("alpha (normalised min-sum) takes EXIT_FIXED or EXIT_PER_FRAME and returns no flag history")
    app = torch.empty((code.N, F), dtype=torch.float32, device=dev) if want_app else None
    hist = torch.zeros(F, dtype=torch.int64, device=dev) if want_flag_hist else None
    it = ctypes.c_int(0)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)
    if alpha is not None:
        iters = torch.empty(F, dtype=torch.int32, device=dev) if exit_mode == EXIT_PER_FRAME else None
        check(lib.bldpc_decode_normalised(code._h, _dev_ptr(Channel_Out), F, int(max_iter), ctypes.c_float(alpha), int(length), int(exit_mode),
                                          int(kernel), _dev_ptr(D), _dev_ptr(app), _dev_ptr(iters), st), "LDPC_Decoder_GPU")
        if iters is not None:
            return dict(D=D, iteraTime=None, app=app, flag_hist=None, iters=iters)
        return dict(D=D, iteraTime=int(max_iter), app=app, flag_hist=None)
    if exit_mode == EXIT_PER_FRAME:
        if want_flag_hist:
            raise ValueError("flag history is not returned with per-frame exit (iters holds each frame's stop iteration)")
        iters = torch.empty(F, dtype=torch.int32, device=dev)
        check(lib.bldpc_decode_per_frame(code._h, _dev_ptr(Channel_Out), F, max_iter, length, kernel, _dev_ptr(D), _dev_ptr(app),
                                         _dev_ptr(iters), st), "LDPC_Decoder_GPU")
        return dict(D=D, iteraTime=None, app=app, flag_hist=None, iters=iters)
    check(lib.bldpc_decode(code._h, _dev_ptr(Channel_Out), F, max_iter, length, exit_mode, kernel, _dev_ptr(D), _dev_ptr(app),
                           _dev_ptr(hist), ctypes.byref(it), st), "LDPC_Decoder_GPU")
    return dict(D=D, iteraTime=it.value, app=app, flag_hist=hist)


def _layered_device(what, fn, code, Channel_Out, max_iter, param, length, exit_mode, stop_rule, D, want_app, app_dtype, stream):
    """What the device wrappers of the row-layered decoders share: the checks of Channel_Out and D, the allocation of D, app and iters,
    the stream, the C call `fn` (all three take the same arguments around the decoder's own parameter, which param() makes once the
    inputs are checked) and the result dict."""
    if not (torch.is_tensor(Channel_Out) and Channel_Out.is_cuda and Channel_Out.dtype == torch.float32 and Channel_Out.is_contiguous()):
        raise ValueError("Channel_Out must be a contiguous CUDA float32 tensor")
    if Channel_Out.dim() != 2 or Channel_Out.shape[0] != code.N or Channel_Out.shape[1] <= 0:
        raise ValueError("Channel_Out must be [N=%d, F]" % code.N)
    F = int(Channel_Out.shape[1])
    dev = Channel_Out.device
    if D is None:
        D = torch.empty((code.N + 1, F), dtype=torch.int32, device=dev)
    else:
        _check_D(D, code.N, F, dev)
    app = torch.empty((code.N, F), dtype=app_dtype, device=dev) if want_app else None
    iters = torch.empty(F, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)
    check(fn(code._h, _dev_ptr(Channel_Out), F, int(max_iter), param(), int(length), int(exit_mode), int(stop_rule), _dev_ptr(D), _dev_ptr(app),
             _dev_ptr(iters), st), what)
    return dict(D=D, app=app, iters=iters)


def _host_statement(what, fn, H, J, L, Z, y, max_iter, param, length, exit_mode, stop_rule, want_app, app_dtype):
    """What the wrappers of the host statements share: the checks of H and y, the allocation of D, app and iters, the C call `fn` (all
    four take the same arguments around the decoder's own parameter, made by param(); stop_rule None: `fn` takes none) and the
    result dict."""
    H = np.ascontiguousarray(H, np.int32)
    if H.size != J * L:
        raise ValueError("H must hold J*L shifts")
    y = np.ascontiguousarray(y, np.float32)
    N = L * Z
    if y.ndim != 2 or y.shape[0] != N or y.shape[1] <= 0:
        raise ValueError("y must be [N=%d, F]" % N)
    F = y.shape[1]
    D = np.zeros((N + 1, F), np.int32)
    app = np.zeros((N, F), app_dtype) if want_app else None
    iters = np.zeros(F, np.int32)
    rule = () if stop_rule is None else (int(stop_rule),)
    check(fn(J, L, Z, _np_ptr(H), _np_ptr(y), F, int(max_iter), param(), int(length), int(exit_mode), *rule, _np_ptr(D),
             None if app is None else _np_ptr(app), _np_ptr(iters)), what)
    return dict(D=D, app=app, iters=iters)


def LDPC_Decoder_Layered_GPU(code, Channel_Out, max_iter=25, alpha=1.0, length=0, exit_mode=EXIT_FIXED, stop_rule=STOP_PREFIX, D=None,
                             want_app=False, stream=None):
    """bldpc_decode_layered: row-layered normalised min-sum (semantics in include/bldpc.h), codes made from block shifts only.

    Channel_Out: CUDA float32 tensor [N, F] (frame-fastest).  alpha in (0, 1] scales every check message (1.0 = plain min-sum).
    stop_rule: STOP_PREFIX (first `length` bits zero, the flooding decoders' rule) or STOP_SYNDROME (H d = 0, any codeword);
    it is what row N of D means and what EXIT_PER_FRAME tests.  EXIT_BATCH_GLOBAL is refused.
    Returns dict(D=int32 [N+1, F], app=float32 [N, F] or None, iters=int32 [F]: iterations run by each frame)."""
    return _layered_device("LDPC_Decoder_Layered_GPU", lib.bldpc_decode_layered, code, Channel_Out, max_iter, lambda: ctypes.c_float(alpha), length,
                           exit_mode, stop_rule, D, want_app, torch.float32, stream)


def layered_host(H, J, L, Z, y, max_iter=25, alpha=1.0, length=0, exit_mode=EXIT_FIXED, stop_rule=STOP_PREFIX, want_app=True):
    """bldpc_decode_layered_host: the layered decoder on the host (no device), the statement of its semantics.  y: float32
    [N, F] host array (frame-fastest).  Returns dict(D=int32 [N+1, F], app=float32 [N, F] or None, iters=int32 [F])."""
    return _host_statement("layered_host", lib.bldpc_decode_layered_host, H, J, L, Z, y, max_iter, lambda: ctypes.c_float(alpha), length, exit_mode,
                           stop_rule, want_app, np.float32)


def LDPC_Decoder_BP_GPU(code, Channel_Out, max_iter=25, llr_scale=1.0, length=0, exit_mode=EXIT_FIXED, stop_rule=STOP_PREFIX, D=None,
                        want_app=False, stream=None):
    """bldpc_decode_layered_bp: row-layered sum-product (box-plus with a 128-entry correction table; semantics in include/bldpc.h),
    codes made from block shifts only.

    Channel_Out: CUDA float32 tensor [N, F] (frame-fastest).  llr_scale turns it into true LLRs: 2 / sigma^2 for the BPSK channels,
    1.0 after Demodulate_QAM with scale 1 / (2 sigma^2).  stop_rule, exit_mode, length and D as in LDPC_Decoder_Layered_GPU.
    Returns dict(D=int32 [N+1, F], app=float32 [N, F] or None, iters=int32 [F]: iterations run by each frame)."""
    return _layered_device("LDPC_Decoder_BP_GPU", lib.bldpc_decode_layered_bp, code, Channel_Out, max_iter, lambda: ctypes.c_float(llr_scale), length,
                           exit_mode, stop_rule, D, want_app, torch.float32, stream)


def bp_host(H, J, L, Z, y, max_iter=25, llr_scale=1.0, length=0, exit_mode=EXIT_FIXED, stop_rule=STOP_PREFIX, want_app=True):
    """bldpc_decode_layered_bp_host: the sum-product decoder on the host (no device), the statement of its semantics.  y: float32
    [N, F] host array (frame-fastest).  Returns dict(D=int32 [N+1, F], app=float32 [N, F] or None, iters=int32 [F])."""
    return _host_statement("bp_host", lib.bldpc_decode_layered_bp_host, H, J, L, Z, y, max_iter, lambda: ctypes.c_float(llr_scale), length, exit_mode,
                           stop_rule, want_app, np.float32)


def BP_Table():
    """bldpc_bp_table: the sum-product decoders' correction table, float32 [128]: T[k] = log1p(exp(-(k + 0.5) / 16)) to the nearest fp32."""
    T = np.zeros(128, np.float32)
    check(lib.bldpc_bp_table(_np_ptr(T)), "BP_Table")
    return T


class Quant:
    """The word lengths of the quantised layered min-sum decoder (struct bldpc_quant, include/bldpc.h), checked as the C side checks
    them (ValueError).

    bits_ch   2 .. bits_app   channel word, saturates at +-C, C = 2^(bits_ch-1) - 1
    bits_app  bits_msg .. 15  a-posteriori word, saturates at +-A, A = 2^(bits_app-1) - 1
    bits_msg  2 .. 8          check-message word, magnitudes saturate at Mx = 2^(bits_msg-1) - 1
    norm8     1 .. 8          normalisation in eighths, rounded: g(m) = max(0, ((m * norm8 + 4) >> 3) - offset); 8 = none
    offset    0 .. Mx         offset subtracted after the normalisation
    llr_scale finite, > 0     quantiser gain: a channel value y becomes rint(llr_scale * y), ties to even

    llr_scale is an absolute gain on the channel value.  Min-sum is scale-invariant, so it only sets the resolution: y = 1.0 (a
    noiseless BPSK symbol) becomes the integer llr_scale.  The smallest of the ~20 magnitudes of a rate-5/6 row is often a few
    units, so a scale below about 16 costs error rate on those codes: on J4_L24_Z96 at sigma 0.52, ten iterations of (6, 8, 6),
    norm8 = 6 leave 14 of 400 frames in error at scale 8 and 9 at scale 16, which is what the fp32 decoder leaves at alpha 0.75."""

    def __init__(self, bits_ch=6, bits_app=8, bits_msg=6, norm8=6, offset=0, llr_scale=16.0):
        ints = dict(bits_ch=bits_ch, bits_app=bits_app, bits_msg=bits_msg, norm8=norm8, offset=offset)
        for k, v in ints.items():
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError("%s must be an integer" % k)
        llr_scale = float(llr_scale)
        if not (np.isfinite(llr_scale) and llr_scale > 0):
            raise ValueError("llr_scale=%r must be finite and positive" % llr_scale)
        if not 2 <= bits_msg <= 8:
            raise ValueError("bits_msg=%d outside [2, 8]" % bits_msg)
        if not bits_msg <= bits_app <= 15:
            raise ValueError("bits_app=%d outside [bits_msg=%d, 15]" % (bits_app, bits_msg))
        if not 2 <= bits_ch <= bits_app:
            raise ValueError("bits_ch=%d outside [2, bits_app=%d]" % (bits_ch, bits_app))
        if not 1 <= norm8 <= 8:
            raise ValueError("norm8=%d outside [1, 8]" % norm8)
        if not 0 <= offset <= (1 << (bits_msg - 1)) - 1:
            raise ValueError("offset=%d outside [0, %d]" % (offset, (1 << (bits_msg - 1)) - 1))
        self.bits_ch, self.bits_app, self.bits_msg, self.norm8, self.offset = (int(v) for v in ints.values())
        self.llr_scale = llr_scale

    @property
    def C(self):
        return (1 << (self.bits_ch - 1)) - 1

    @property
    def A(self):
        return (1 << (self.bits_app - 1)) - 1

    @property
    def Mx(self):
        return (1 << (self.bits_msg - 1)) - 1

    def c_struct(self):
        return bldpc_quant(self.llr_scale, self.bits_ch, self.bits_app, self.bits_msg, self.norm8, self.offset)

    def __repr__(self):
        return "Quant(bits_ch=%d, bits_app=%d, bits_msg=%d, norm8=%d, offset=%d, llr_scale=%g)" % (
            self.bits_ch, self.bits_app, self.bits_msg, self.norm8, self.offset, self.llr_scale)


def _quant_ref(quant):
    """byref of the C struct of a Quant; a raw _lib.bldpc_quant passes unchecked (the C side checks it) and None is the null pointer."""
    if quant is None:
        return None
    if isinstance(quant, bldpc_quant):
        return ctypes.byref(quant)
    if not isinstance(quant, Quant):
        raise ValueError("quant must be a cuda_ldpc_amd.Quant")
    return ctypes.byref(quant.c_struct())


def LDPC_Decoder_Quant_GPU(code, Channel_Out, quant, max_iter=25, length=0, exit_mode=EXIT_FIXED, stop_rule=STOP_PREFIX, D=None,
                           want_app=False, stream=None):
    """bldpc_decode_layered_quant: row-layered min-sum with finite word lengths (semantics in include/bldpc.h; Quant explains the
    parameters and llr_scale), two frames per packed 16-bit instruction, codes made from block shifts only.

    Channel_Out: CUDA float32 tensor [N, F] (frame-fastest).  stop_rule, exit_mode, length and D as in LDPC_Decoder_Layered_GPU.
    Returns dict(D=int32 [N+1, F], app=int32 [N, F] or None: the a-posteriori words, iters=int32 [F]: iterations run by each frame)."""
    return _layered_device("LDPC_Decoder_Quant_GPU", lib.bldpc_decode_layered_quant, code, Channel_Out, max_iter, lambda: _quant_ref(quant), length,
                           exit_mode, stop_rule, D, want_app, torch.int32, stream)


def quant_host(H, J, L, Z, y, quant, max_iter=25, length=0, exit_mode=EXIT_FIXED, stop_rule=STOP_PREFIX, want_app=True):
    """bldpc_decode_layered_quant_host: the quantised layered decoder on the host (no device), the statement of its semantics.
    y: float32 [N, F] host array (frame-fastest).  Returns dict(D=int32 [N+1, F], app=int32 [N, F] or None, iters=int32 [F])."""
    return _host_statement("quant_host", lib.bldpc_decode_layered_quant_host, H, J, L, Z, y, max_iter, lambda: _quant_ref(quant), length, exit_mode,
                           stop_rule, want_app, np.int32)


# ---- hard-decision decoding: packed hard bits, the binary symmetric channel, bit flipping (bldpc.h) ----------------------------------------
def _words(F):
    return (int(F) + 31) // 32


def _check_bits(bits, rows, F, dev=None):
    """Packed hard bits [rows, ceil(F/32)] as the C ABI reads them: int32 words (torch has no uint32 arithmetic; the bits are the same)."""
    W = _words(F)
    if dev is None:
        a = np.ascontiguousarray(bits)
        if a.dtype not in (np.uint32, np.int32) or a.shape != (rows, W):
            raise ValueError("bits must be a uint32 array [%d, %d]" % (rows, W))
        return a.view(np.uint32)
    if not (torch.is_tensor(bits) and bits.is_cuda and bits.dtype == torch.int32 and bits.is_contiguous() and tuple(bits.shape) == (rows, W)):
        raise ValueError("bits must be a contiguous CUDA int32 tensor [%d, %d]" % (rows, W))
    return bits


def _pack_device(what, fn, src, dtype, stream):
    if not (torch.is_tensor(src) and src.is_cuda and src.dtype == dtype and src.is_contiguous() and src.dim() == 2 and src.numel() > 0):
        raise ValueError("%s needs a contiguous CUDA %s tensor [rows, F]" % (what, dtype))
    rows, F = (int(x) for x in src.shape)
    bits = torch.empty((rows, _words(F)), dtype=torch.int32, device=src.device)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(src.device)).cuda_stream)
    check(fn(_dev_ptr(src), rows, F, _dev_ptr(bits), st), what)
    return bits


def Hard_Pack(Channel_Out, stream=None):
    """bldpc_hard_pack: the hard decisions of Channel_Out (CUDA float32 [N, F]) as packed bits, CUDA int32 [N, ceil(F/32)]: frame f is
    bit f % 32 of word f // 32, the bit is Channel_Out < 0 (-0.0 and NaN give 0), padding bits are 0."""
    return _pack_device("Hard_Pack", lib.bldpc_hard_pack, Channel_Out, torch.float32, stream)


def Hard_Pack_Int(CodeWord, stream=None):
    """bldpc_hard_pack_int: the same layout from int32 bits [rows, F], the bit is != 0."""
    return _pack_device("Hard_Pack_Int", lib.bldpc_hard_pack_int, CodeWord, torch.int32, stream)


def Hard_Unpack(bits, F, stream=None):
    """bldpc_hard_unpack: packed bits (CUDA int32 [rows, ceil(F/32)]) -> CUDA int32 [rows, F] of 0 and 1."""
    if not (torch.is_tensor(bits) and bits.dim() == 2 and F > 0):
        raise ValueError("bits must be a CUDA int32 tensor [rows, ceil(F/32)] and F > 0")
    rows = int(bits.shape[0])
    _check_bits(bits, rows, F, bits.device)
    D = torch.empty((rows, int(F)), dtype=torch.int32, device=bits.device)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(bits.device)).cuda_stream)
    check(lib.bldpc_hard_unpack(_dev_ptr(bits), rows, int(F), _dev_ptr(D), st), "Hard_Unpack")
    return D


def _pack_host(what, fn, src, dtype):
    a = np.ascontiguousarray(src, dtype)
    if a.ndim != 2 or a.size == 0:
        raise ValueError("%s needs an array [rows, F]" % what)
    bits = np.empty((a.shape[0], _words(a.shape[1])), np.uint32)
    check(fn(_np_ptr(a), a.shape[0], a.shape[1], _np_ptr(bits)), what)
    return bits


def Hard_Pack_host(Channel_Out):
    """bldpc_hard_pack_host: Hard_Pack over a host float32 array [N, F]; returns uint32 [N, ceil(F/32)]."""
    return _pack_host("Hard_Pack_host", lib.bldpc_hard_pack_host, Channel_Out, np.float32)


def Hard_Pack_Int_host(CodeWord):
    """bldpc_hard_pack_int_host: Hard_Pack_Int over a host int32 array [rows, F]."""
    return _pack_host("Hard_Pack_Int_host", lib.bldpc_hard_pack_int_host, CodeWord, np.int32)


def Hard_Unpack_host(bits, F):
    """bldpc_hard_unpack_host: packed host bits [rows, ceil(F/32)] -> int32 [rows, F]."""
    bits = np.ascontiguousarray(bits)
    if bits.ndim != 2 or F <= 0:
        raise ValueError("bits must be [rows, ceil(F/32)] and F > 0")
    bits = _check_bits(bits, bits.shape[0], F)
    D = np.empty((bits.shape[0], int(F)), np.int32)
    check(lib.bldpc_hard_unpack_host(_np_ptr(bits), bits.shape[0], int(F), _np_ptr(D)), "Hard_Unpack_host")
    return D


def _check_bsc(seed, p):
    if not (isinstance(seed, np.ndarray) and seed.dtype == np.int32 and seed.size == 3):
        raise ValueError("seed must be an int32 numpy array of 3")
    if not (np.isfinite(p) and 0.0 <= p <= 0.5):
        raise ValueError("p must be a crossover probability in [0, 0.5], not %r" % (p,))


def BSCChannel_CPU(seed, p, N, F, CodeWord=None):
    """bldpc_bsc_channel_host: the binary symmetric channel over the RandomModule stream.  Bit (f, n) is CodeWord[n, f] (None: the all-zero
    word) flipped iff draw f * N + n is below p (a float32 compare).  seed (int32[3]) advances by N * F draws.  Returns packed bits,
    uint32 [N, ceil(F/32)]."""
    _check_bsc(seed, p)
    cw = None if CodeWord is None else np.ascontiguousarray(CodeWord, np.int32)
    if cw is not None and cw.shape != (N, F):
        raise ValueError("CodeWord must be [N=%d, F=%d]" % (N, F))
    bits = np.empty((N, _words(F)), np.uint32)
    check(lib.bldpc_bsc_channel_host(_np_ptr(seed), ctypes.c_float(p), None if cw is None else _np_ptr(cw), N, F, _np_ptr(bits)), "BSCChannel_CPU")
    return bits


def BSCChannel_GPU(seed, p, N, F, device=None, CodeWord=None, stream=None):
    """bldpc_bsc_channel_device: the same channel and the same draws on the device.  CodeWord: CUDA int32 [N, F] or None.  Returns
    packed bits, CUDA int32 [N, ceil(F/32)]; seed advanced."""
    _check_bsc(seed, p)
    device = device or (CodeWord.device if CodeWord is not None else torch.device("cuda", torch.cuda.current_device()))
    if CodeWord is not None and not (torch.is_tensor(CodeWord) and CodeWord.is_cuda and CodeWord.dtype == torch.int32 and CodeWord.is_contiguous()
                                     and tuple(CodeWord.shape) == (N, F)):
        raise ValueError("CodeWord must be a contiguous CUDA int32 tensor [N=%d, F=%d]" % (N, F))
    bits = torch.empty((N, _words(F)), dtype=torch.int32, device=device)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(device)).cuda_stream)
    check(lib.bldpc_bsc_channel_device(_np_ptr(seed), ctypes.c_float(p), _dev_ptr(CodeWord), N, F, _dev_ptr(bits), st), "BSCChannel_GPU")
    return bits


def LDPC_Decoder_BitFlip_GPU(code, bits, F, rule=BF_GRADIENT, max_iter=30, exit_mode=EXIT_FIXED, D=None, want_bits=False, stream=None, want_D=True):
    """bldpc_decode_bitflip: hard-decision decoding by parallel bit flipping (semantics in include/bldpc.h), 32 frames in the bits of a
    word, all iterations on-chip (k_bf).  bits: packed received bits, CUDA int32 [N, ceil(F/32)] (Hard_Pack, BSCChannel_GPU).
    rule: BF_THRESHOLD (flip iff 2 u + e > d) or BF_GRADIENT (flip the variables of largest u + e).  EXIT_FIXED or EXIT_PER_FRAME.
    Returns dict(D=int32 [N+1, F] with row N the syndrome flag, or None with want_D=False; Dbits=int32 [N+1, ceil(F/32)] or None;
    iters=int32 [F])."""
    if not isinstance(F, (int, np.integer)) or F <= 0:
        raise ValueError("F must be a positive int")
    if not (torch.is_tensor(bits) and bits.is_cuda):
        raise ValueError("bits must be a CUDA int32 tensor [N, ceil(F/32)]")
    dev = bits.device
    _check_bits(bits, code.N, F, dev)
    if D is not None:
        _check_D(D, code.N, F, dev)
    elif want_D:
        D = torch.empty((code.N + 1, F), dtype=torch.int32, device=dev)
    elif not want_bits:
        raise ValueError("want_D=False needs want_bits=True: the call must have an output")
    Dbits = torch.empty((code.N + 1, _words(F)), dtype=torch.int32, device=dev) if want_bits else None
    iters = torch.empty(F, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)
    check(lib.bldpc_decode_bitflip(code._h, _dev_ptr(bits), int(F), int(max_iter), int(rule), int(exit_mode), _dev_ptr(D), _dev_ptr(Dbits),
                                   _dev_ptr(iters), st), "LDPC_Decoder_BitFlip_GPU")
    return dict(D=D, Dbits=Dbits, iters=iters)


def bitflip_host(H, J, L, Z, bits, F, rule=BF_GRADIENT, max_iter=30, exit_mode=EXIT_FIXED):
    """bldpc_decode_bitflip_host: the bit-flipping decoder on the host (no device), the statement of its semantics.  bits: uint32
    [N, ceil(F/32)].  Returns dict(D=int32 [N+1, F], Dbits=uint32 [N+1, ceil(F/32)], iters=int32 [F])."""
    H = np.ascontiguousarray(H, np.int32)
    if H.size != J * L:
        raise ValueError("H must hold J*L shifts")
    if not isinstance(F, (int, np.integer)) or F <= 0:
        raise ValueError("F must be a positive int")
    N = L * Z
    bits = _check_bits(bits, N, F)
    D = np.zeros((N + 1, F), np.int32)
    Dbits = np.zeros((N + 1, _words(F)), np.uint32)
    iters = np.zeros(F, np.int32)
    check(lib.bldpc_decode_bitflip_host(J, L, Z, _np_ptr(H), _np_ptr(bits), int(F), int(max_iter), int(rule), int(exit_mode), _np_ptr(D),
                                        _np_ptr(Dbits), _np_ptr(iters)), "bitflip_host")
    return dict(D=D, Dbits=Dbits, iters=iters)


def bitflip_plan_host(H, J, L, Z):
    """bldpc_bitflip_plan_host: what BinaryCode.bitflip_info returns, from the block matrix alone (no device)."""
    H = np.ascontiguousarray(H, np.int32)
    if H.size != J * L:
        raise ValueError("H must hold J*L shifts")
    d = np.zeros(4, np.int32)
    check(lib.bldpc_bitflip_plan_host(J, L, Z, _np_ptr(H), _np_ptr(d)), "bitflip_plan_host")
    return dict(lds_bytes=int(d[0]), threads=int(d[1]), frames_per_wg=int(d[2]), fits=int(d[0]) <= BITFLIP_LDS_BOUND)


# ---- erasure decoding: erased words, the binary erasure channel, peeling, statistics on packed words (bldpc.h) ----------------------------
ERASURE_LDS_BOUND = BITFLIP_LDS_BOUND  # k_er's state, 4 (2 N + M) bytes, against the same bound


def _check_bec(seed, p):
    if not (isinstance(seed, np.ndarray) and seed.dtype == np.int32 and seed.size == 3):
        raise ValueError("seed must be an int32 numpy array of 3")
    if not (np.isfinite(p) and 0.0 <= p <= 1.0):
        raise ValueError("p must be an erasure probability in [0, 1], not %r" % (p,))


def BECChannel_CPU(seed, p, N, F, CodeWord=None):
    """bldpc_bec_channel_host: the binary erasure channel over the RandomModule stream.  Bit (f, n) is erased iff draw f * N + n is
    below p (the BSC's indexing and float32 compare); bits = CodeWord (None: the all-zero word) with 0 at the erased positions.  seed
    (int32[3]) advances by N * F draws.  Returns (bits, erased), uint32 [N, ceil(F/32)] each."""
    _check_bec(seed, p)
    cw = None if CodeWord is None else np.ascontiguousarray(CodeWord, np.int32)
    if cw is not None and cw.shape != (N, F):
        raise ValueError("CodeWord must be [N=%d, F=%d]" % (N, F))
    bits, erased = np.empty((N, _words(F)), np.uint32), np.empty((N, _words(F)), np.uint32)
    check(lib.bldpc_bec_channel_host(_np_ptr(seed), ctypes.c_float(p), None if cw is None else _np_ptr(cw), N, F, _np_ptr(bits), _np_ptr(erased)),
          "BECChannel_CPU")
    return bits, erased


def BECChannel_GPU(seed, p, N, F, device=None, CodeWord=None, stream=None):
    """bldpc_bec_channel_device: the same channel and the same draws on the device.  CodeWord: CUDA int32 [N, F] or None.  Returns
    (bits, erased), CUDA int32 [N, ceil(F/32)] each; seed advanced."""
    _check_bec(seed, p)
    device = device or (CodeWord.device if CodeWord is not None else torch.device("cuda", torch.cuda.current_device()))
    if CodeWord is not None and not (torch.is_tensor(CodeWord) and CodeWord.is_cuda and CodeWord.dtype == torch.int32 and CodeWord.is_contiguous()
                                     and tuple(CodeWord.shape) == (N, F)):
        raise ValueError("CodeWord must be a contiguous CUDA int32 tensor [N=%d, F=%d]" % (N, F))
    bits = torch.empty((N, _words(F)), dtype=torch.int32, device=device)
    erased = torch.empty((N, _words(F)), dtype=torch.int32, device=device)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(device)).cuda_stream)
    check(lib.bldpc_bec_channel_device(_np_ptr(seed), ctypes.c_float(p), _dev_ptr(CodeWord), N, F, _dev_ptr(bits), _dev_ptr(erased), st),
          "BECChannel_GPU")
    return bits, erased


def LDPC_Decoder_Erasure_GPU(code, bits, erased, F, max_iter=100, D=None, want_bits=True, want_erased=True, want_D=False, stream=None):
    """bldpc_decode_erasure: parallel peeling on the erasure channel (semantics in include/bldpc.h), 32 frames in the bits of a word, all
    iterations on-chip (k_er).  bits, erased: CUDA int32 [N, ceil(F/32)] (BECChannel_GPU, RM_Recover_Bits).  Returns dict(D=int32
    [N+1, F] with row N the flag, given or with want_D=True, else None; Dbits=int32 [N+1, ceil(F/32)] or None; Ebits=int32
    [N, ceil(F/32)], the residual mask, or None; iters=int32 [F], the last productive iteration of every frame)."""
    if not isinstance(F, (int, np.integer)) or F <= 0:
        raise ValueError("F must be a positive int")
    if not (torch.is_tensor(bits) and bits.is_cuda and torch.is_tensor(erased) and erased.is_cuda and erased.device == bits.device):
        raise ValueError("bits and erased must be CUDA int32 tensors [N, ceil(F/32)] on one device")
    dev = bits.device
    _check_bits(bits, code.N, F, dev)
    _check_bits(erased, code.N, F, dev)
    if D is not None:
        _check_D(D, code.N, F, dev)
    elif want_D:
        D = torch.empty((code.N + 1, F), dtype=torch.int32, device=dev)
    elif not (want_bits or want_erased):
        raise ValueError("the call must have an output: D, want_D, want_bits or want_erased")
    Dbits = torch.empty((code.N + 1, _words(F)), dtype=torch.int32, device=dev) if want_bits else None
    Ebits = torch.empty((code.N, _words(F)), dtype=torch.int32, device=dev) if want_erased else None
    iters = torch.empty(F, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)
    check(lib.bldpc_decode_erasure(code._h, _dev_ptr(bits), _dev_ptr(erased), int(F), int(max_iter), _dev_ptr(D), _dev_ptr(Dbits), _dev_ptr(Ebits),
                                   _dev_ptr(iters), st), "LDPC_Decoder_Erasure_GPU")
    return dict(D=D, Dbits=Dbits, Ebits=Ebits, iters=iters)


def erasure_host(H, J, L, Z, bits, erased, F, max_iter=100):
    """bldpc_decode_erasure_host: the peeling decoder on the host (no device), the statement of its semantics.  bits, erased: uint32
    [N, ceil(F/32)].  Returns dict(D=int32 [N+1, F], Dbits=uint32 [N+1, ceil(F/32)], Ebits=uint32 [N, ceil(F/32)], iters=int32 [F])."""
    H = np.ascontiguousarray(H, np.int32)
    if H.size != J * L:
        raise ValueError("H must hold J*L shifts")
    if not isinstance(F, (int, np.integer)) or F <= 0:
        raise ValueError("F must be a positive int")
    N = L * Z
    bits, erased = _check_bits(bits, N, F), _check_bits(erased, N, F)
    D = np.zeros((N + 1, F), np.int32)
    Dbits = np.zeros((N + 1, _words(F)), np.uint32)
    Ebits = np.zeros((N, _words(F)), np.uint32)
    iters = np.zeros(F, np.int32)
    check(lib.bldpc_decode_erasure_host(J, L, Z, _np_ptr(H), _np_ptr(bits), _np_ptr(erased), int(F), int(max_iter), _np_ptr(D), _np_ptr(Dbits),
                                        _np_ptr(Ebits), _np_ptr(iters)), "erasure_host")
    return dict(D=D, Dbits=Dbits, Ebits=Ebits, iters=iters)


def erasure_plan_host(H, J, L, Z):
    """bldpc_erasure_plan_host: what BinaryCode.erasure_info returns, from the block matrix alone (no device)."""
    H = np.ascontiguousarray(H, np.int32)
    if H.size != J * L:
        raise ValueError("H must hold J*L shifts")
    d = np.zeros(4, np.int32)
    check(lib.bldpc_erasure_plan_host(J, L, Z, _np_ptr(H), _np_ptr(d)), "erasure_plan_host")
    return dict(lds_bytes=int(d[0]), threads=int(d[1]), frames_per_wg=int(d[2]), fits=int(d[0]) <= ERASURE_LDS_BOUND)


# ---- erasure decoding by elimination (bldpc.h): the maximum-likelihood decoder of the erasure channel ------------------------------------
ML_NONE, ML_SOLVED, ML_PARTIAL, ML_STUCK, ML_INCONSISTENT, ML_SKIPPED = range(6)  # status of a frame
ML_TIERS = {"auto": 0, "lds": 1, "workspace": 2}


def _ml_tier(tier):
    if tier not in ML_TIERS:
        raise ValueError("tier must be one of %s, not %r" % (sorted(ML_TIERS), tier))
    return ML_TIERS[tier]


def _ml_info(d):
    return dict(matrix_bytes=int(d[0]), threads=int(d[1]), tier={1: "lds", 2: "workspace"}.get(int(d[2])), slots=int(d[3]))


def LDPC_Decoder_Erasure_ML_GPU(code, bits, erased, F, max_erased=0, tier="auto", D=None, want_bits=True, want_erased=True, want_D=False,
                                stream=None):
    """bldpc_decode_erasure_ml: maximum-likelihood decoding on the erasure channel (semantics in include/bldpc.h): per frame the linear
    system the erased positions leave is reduced over GF(2), one workgroup a frame (k_er_ml, or k_er_ml_ws with the matrix in a workspace
    slot).  bits, erased: CUDA int32 [N, ceil(F/32)], typically the first N rows of a peeling Dbits and its Ebits.  Frames with more
    than max_erased erasures (0: M) are left as they came.  Returns dict(D=int32 [N+1, F] with row N the flag, given or with want_D=True,
    else None; Dbits=int32 [N+1, ceil(F/32)] or None; Ebits=int32 [N, ceil(F/32)] or None; status=int32 [F], ML_NONE .. ML_SKIPPED;
    rank=int32 [F], the rank of the frame's system, -1 where skipped)."""
    if not isinstance(F, (int, np.integer)) or F <= 0:
        raise ValueError("F must be a positive int")
    if not (torch.is_tensor(bits) and bits.is_cuda and torch.is_tensor(erased) and erased.is_cuda and erased.device == bits.device):
        raise ValueError("bits and erased must be CUDA int32 tensors [N, ceil(F/32)] on one device")
    dev = bits.device
    _check_bits(bits, code.N, F, dev)
    _check_bits(erased, code.N, F, dev)
    t = _ml_tier(tier)
    if D is not None:
        _check_D(D, code.N, F, dev)
    elif want_D:
        D = torch.empty((code.N + 1, F), dtype=torch.int32, device=dev)
    elif not (want_bits or want_erased):
        raise ValueError("the call must have an output: D, want_D, want_bits or want_erased")
    Dbits = torch.empty((code.N + 1, _words(F)), dtype=torch.int32, device=dev) if want_bits else None
    Ebits = torch.empty((code.N, _words(F)), dtype=torch.int32, device=dev) if want_erased else None
    status = torch.empty(F, dtype=torch.int32, device=dev)
    rank = torch.empty(F, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)
    check(lib.bldpc_decode_erasure_ml(code._h, _dev_ptr(bits), _dev_ptr(erased), int(F), int(max_erased), t, _dev_ptr(D), _dev_ptr(Dbits),
                                      _dev_ptr(Ebits), _dev_ptr(status), _dev_ptr(rank), st), "LDPC_Decoder_Erasure_ML_GPU")
    return dict(D=D, Dbits=Dbits, Ebits=Ebits, status=status, rank=rank)


def erasure_ml_host(H, J, L, Z, bits, erased, F, max_erased=0):
    """bldpc_decode_erasure_ml_host: the elimination decoder on the host (no device), the statement of its semantics.  bits, erased:
    uint32 [N, ceil(F/32)].  Returns dict(D=int32 [N+1, F], Dbits=uint32 [N+1, ceil(F/32)], Ebits=uint32 [N, ceil(F/32)], status=int32
    [F], rank=int32 [F])."""
    H = np.ascontiguousarray(H, np.int32)
    if H.size != J * L:
        raise ValueError("H must hold J*L shifts")
    if not isinstance(F, (int, np.integer)) or F <= 0:
        raise ValueError("F must be a positive int")
    N = L * Z
    bits, erased = _check_bits(bits, N, F), _check_bits(erased, N, F)
    D = np.zeros((N + 1, F), np.int32)
    Dbits = np.zeros((N + 1, _words(F)), np.uint32)
    Ebits = np.zeros((N, _words(F)), np.uint32)
    status, rank = np.zeros(F, np.int32), np.zeros(F, np.int32)
    check(lib.bldpc_decode_erasure_ml_host(J, L, Z, _np_ptr(H), _np_ptr(bits), _np_ptr(erased), int(F), int(max_erased), _np_ptr(D), _np_ptr(Dbits),
                                           _np_ptr(Ebits), _np_ptr(status), _np_ptr(rank)), "erasure_ml_host")
    return dict(D=D, Dbits=Dbits, Ebits=Ebits, status=status, rank=rank)


def erasure_ml_plan_host(H, J, L, Z, max_erased=0, tier="auto"):
    """bldpc_erasure_ml_plan_host: what BinaryCode.erasure_ml_info returns, from the block matrix alone (no device; the 256 compute units
    of an MI355X).  A refusal (LdpcError) is the one the device call would make."""
    H = np.ascontiguousarray(H, np.int32)
    if H.size != J * L:
        raise ValueError("H must hold J*L shifts")
    d = np.zeros(4, np.int32)
    check(lib.bldpc_erasure_ml_plan_host(J, L, Z, _np_ptr(H), int(max_erased), _ml_tier(tier), _np_ptr(d)), "erasure_ml_plan_host")
    return _ml_info(d)


# ---- ordered-statistics reprocessing (bldpc.h): OSD-0 on the frames a soft decoder leaves with a non-zero syndrome --------------------------
def _osd_info(d):
    return dict(lds_bytes=int(d[0]), threads=int(d[1]), tier={1: "lds", 2: "workspace"}.get(int(d[2])), slots=int(d[3]))


def LDPC_Decoder_OSD_GPU(code, app, D=None, tier="auto", out=None, stream=None, order=0, lam=0, want_metric=False):
    """bldpc_decode_osd: ordered-statistics reprocessing of order 0 (semantics in include/bldpc.h): per processed frame the least
    reliable basis of H's columns is found by elimination in the order of |app|, the hard decisions of app are kept outside it and
    re-derived from the parity checks on it, so the frame comes out a codeword with flag 1; one workgroup a frame (k_osd, or k_osd_ws
    with the record of the row operations in a workspace slot).  app: CUDA float32 [N, F], a decoder's app or a channel array.  D: a
    decoder's D, CUDA int32 [N+1, F]: the frames whose flag row is 0 are processed, the others kept; None processes every frame.
    out: where the result goes, CUDA int32 [N+1, F]; default D itself (in place), or a new tensor when D is None.
    Returns (D, flips, scanned): the result, and int32 [F] each the number of hard decisions changed (-1 on a kept frame) and the
    1-based place in the order of reliability of the last basis position (0 on a kept frame).
    order = 1 or 2 (bldpc_decode_osd_w, kernels k_osd_w / k_osd_w_ws): also every single position outside the basis flipped and, at
    order 2, every pair among the first `lam` of them in the order of reliability; the candidate of least soft metric is the result.
    Returns (D, flips, scanned, picked, metric): picked int32 [2, F], the positions flipped outside the basis or -1 (-1, -1 on a kept
    frame), metric float32 [F], the metric of the candidate chosen (not written on a kept frame).  want_metric=True takes order 0
    through the same call, for its metric."""
    if not (torch.is_tensor(app) and app.is_cuda and app.dtype == torch.float32 and app.is_contiguous() and app.dim() == 2
            and app.shape[0] == code.N and app.shape[1] > 0):
        raise ValueError("app must be a contiguous CUDA float32 tensor [N=%d, F]" % code.N)
    dev, F = app.device, int(app.shape[1])
    t = _ml_tier(tier)
    if D is not None:
        _check_D(D, code.N, F, dev)
    if out is None:
        out = D if D is not None else torch.empty((code.N + 1, F), dtype=torch.int32, device=dev)
    else:
        _check_D(out, code.N, F, dev)
    flips = torch.empty(F, dtype=torch.int32, device=dev)
    scanned = torch.empty(F, dtype=torch.int32, device=dev)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)
    if order or want_metric:
        picked = torch.empty((2, F), dtype=torch.int32, device=dev)
        metric = torch.empty(F, dtype=torch.float32, device=dev)
        check(lib.bldpc_decode_osd_w(code._h, _dev_ptr(app), _dev_ptr(D), F, t, int(order), int(lam), _dev_ptr(out), _dev_ptr(flips),
                                     _dev_ptr(scanned), _dev_ptr(picked), _dev_ptr(metric), st), "LDPC_Decoder_OSD_GPU")
        return out, flips, scanned, picked, metric
    check(lib.bldpc_decode_osd(code._h, _dev_ptr(app), _dev_ptr(D), F, t, _dev_ptr(out), _dev_ptr(flips), _dev_ptr(scanned), st), "LDPC_Decoder_OSD_GPU")
    return out, flips, scanned


def osd_host(H, J, L, Z, app, D=None, order=0, lam=0, want_metric=False):
    """bldpc_decode_osd_host: ordered-statistics reprocessing on the host (no device), the statement of its semantics.  app: float32
    [N, F]; D: int32 [N+1, F] or None, as in LDPC_Decoder_OSD_GPU (it is not written).  Returns (D int32 [N+1, F], flips int32 [F],
    scanned int32 [F]); with order >= 1 or want_metric (bldpc_decode_osd_w_host) also picked int32 [2, F] and metric float32 [F], which
    is zero on a kept frame."""
    H = np.ascontiguousarray(H, np.int32)
    if H.size != J * L:
        raise ValueError("H must hold J*L shifts")
    N = L * Z
    app = np.ascontiguousarray(app)
    if app.dtype != np.float32 or app.ndim != 2 or app.shape[0] != N or app.shape[1] < 1:
        raise ValueError("app must be a float32 array [N=%d, F]" % N)
    F = int(app.shape[1])
    if D is not None:
        D = np.ascontiguousarray(D)
        if D.dtype != np.int32 or D.shape != (N + 1, F):
            raise ValueError("D must be an int32 array [N+1=%d, F=%d]" % (N + 1, F))
    out = np.zeros((N + 1, F), np.int32)
    flips, scanned = np.zeros(F, np.int32), np.zeros(F, np.int32)
    if order or want_metric:
        picked, metric = np.zeros((2, F), np.int32), np.zeros(F, np.float32)
        check(lib.bldpc_decode_osd_w_host(J, L, Z, _np_ptr(H), _np_ptr(app), None if D is None else _np_ptr(D), F, int(order), int(lam), _np_ptr(out),
                                          _np_ptr(flips), _np_ptr(scanned), _np_ptr(picked), _np_ptr(metric)), "osd_host")
        return out, flips, scanned, picked, metric
    check(lib.bldpc_decode_osd_host(J, L, Z, _np_ptr(H), _np_ptr(app), None if D is None else _np_ptr(D), F, _np_ptr(out), _np_ptr(flips),
                                    _np_ptr(scanned)), "osd_host")
    return out, flips, scanned


def osd_plan_host(H, J, L, Z, tier="auto", order=0):
    """bldpc_osd_plan_host: what BinaryCode.osd_info returns, from the block matrix alone (no device; the 256 compute units of an
    MI355X).  A refusal (LdpcError) is the one the device call would make.  order >= 1: bldpc_osd_w_plan_host."""
    H = np.ascontiguousarray(H, np.int32)
    if H.size != J * L:
        raise ValueError("H must hold J*L shifts")
    d = np.zeros(4, np.int32)
    if order:
        check(lib.bldpc_osd_w_plan_host(J, L, Z, _np_ptr(H), _ml_tier(tier), int(order), _np_ptr(d)), "osd_plan_host")
        return _osd_info(d)
    check(lib.bldpc_osd_plan_host(J, L, Z, _np_ptr(H), _ml_tier(tier), _np_ptr(d)), "osd_plan_host")
    return _osd_info(d)


def Statistic_Bits(code, Dbits, F, counters, Ebits=None, CodeWordBits=None, iters=None, length=0, stream=None):
    """bldpc_statistic_bits: the five counters of the sweeps (error frames, error bits, iterations, false frames, alarm frames)
    accumulated into `counters` (CUDA int64, at least 5) from packed words: Dbits int32 [N+1, ceil(F/32)] with row N the flag, Ebits the
    residual mask [N, ceil(F/32)] or None, CodeWordBits the packed sent words [>= length rows, ceil(F/32)] or None for the all-zero word,
    iters int32 [F] or None.  A position still erased is a bit error.  length: the rows counted, 0 = code.K."""
    if not isinstance(F, (int, np.integer)) or F <= 0:
        raise ValueError("F must be a positive int")
    if not (torch.is_tensor(Dbits) and Dbits.is_cuda):
        raise ValueError("Dbits must be a CUDA int32 tensor [N+1, ceil(F/32)]")
    dev = Dbits.device
    _check_bits(Dbits, code.N + 1, F, dev)
    if Ebits is not None:
        _check_bits(Ebits, code.N, F, dev)
    if length < 0 or length > code.N:
        raise ValueError("length must lie in [0, N=%d]" % code.N)
    rows = length or code.K
    if CodeWordBits is not None and not (torch.is_tensor(CodeWordBits) and CodeWordBits.dim() == 2 and CodeWordBits.shape[0] >= rows):
        raise ValueError("CodeWordBits must hold at least %d rows" % rows)
    if CodeWordBits is not None:
        _check_bits(CodeWordBits, int(CodeWordBits.shape[0]), F, dev)
    if iters is not None and not (torch.is_tensor(iters) and iters.is_cuda and iters.dtype == torch.int32 and iters.is_contiguous() and iters.numel() >= F):
        raise ValueError("iters must be a contiguous CUDA int32 tensor of at least F=%d" % F)
    _check_counters(counters, 5, dev)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)
    check(lib.bldpc_statistic_bits(code._h, _dev_ptr(Dbits), _dev_ptr(Ebits), _dev_ptr(CodeWordBits), int(F), int(length), _dev_ptr(iters),
                                   _dev_ptr(counters), st), "Statistic_Bits")
    return counters


def Statistic_Bits_host(N, Dbits, F, length, Ebits=None, CodeWordBits=None, iters=None, counters=None):
    """bldpc_statistic_bits_host: Statistic_Bits over host arrays, N in place of the code object and a length in [1, N].  Accumulates
    into `counters` (int64 [5]; None: zeros) and returns it."""
    Dbits = _check_bits(Dbits, N + 1, F)
    Ebits = None if Ebits is None else _check_bits(Ebits, N, F)
    if CodeWordBits is not None:
        CodeWordBits = np.ascontiguousarray(CodeWordBits)
        if CodeWordBits.ndim != 2 or CodeWordBits.shape[0] < length:
            raise ValueError("CodeWordBits must hold at least %d rows" % length)
        CodeWordBits = _check_bits(CodeWordBits, CodeWordBits.shape[0], F)
    if iters is not None:
        iters = np.ascontiguousarray(iters, np.int32)
        if iters.size < F:
            raise ValueError("iters must hold F=%d counts" % F)
    counters = np.zeros(5, np.int64) if counters is None else counters
    if not (isinstance(counters, np.ndarray) and counters.dtype == np.int64 and counters.size >= 5 and counters.flags.c_contiguous):
        raise ValueError("counters must be a contiguous int64 array of at least 5")
    ptr = lambda a: None if a is None else _np_ptr(a)  # noqa: E731
    check(lib.bldpc_statistic_bits_host(int(N), ptr(Dbits), ptr(Ebits), ptr(CodeWordBits), int(F), int(length), ptr(iters), _np_ptr(counters)),
          "Statistic_Bits_host")
    return counters


def normalised_host(H, J, L, Z, y, max_iter=50, alpha=1.0, length=0, exit_mode=EXIT_FIXED, want_app=True):
    """bldpc_decode_normalised_host: the flooding decoder with normalised min-sum on the host (no device), the statement of its
    semantics.  y: float32 [N, F] host array (frame-fastest).  Returns dict(D=int32 [N+1, F], app=float32 [N, F] or None,
    iters=int32 [F]: iterations run by each frame)."""
    return _host_statement("normalised_host", lib.bldpc_decode_normalised_host, H, J, L, Z, y, max_iter, lambda: ctypes.c_float(alpha), length,
                           exit_mode, None, want_app, np.float32)


def _qam_bits(q):
    """log2 q for a constellation size the modem takes (a power of two in 2..256)."""
    q = int(q)
    if q < 2 or q > 256 or q & (q - 1):
        raise ValueError("the constellation must hold a power of two of points in 2..256, not %d" % q)
    return q.bit_length() - 1


def _check_con(constellation, dev=None):
    """constellation [q, 2] float32: a contiguous CUDA tensor on `dev`, or (dev None) anything numpy reads.  Returns (tensor or array, m)."""
    if dev is None:
        con = np.ascontiguousarray(constellation, np.float32)
        if con.ndim != 2 or con.shape[1] != 2:
            raise ValueError("constellation must be float32 [q, 2]")
        return con, _qam_bits(con.shape[0])
    if not (torch.is_tensor(constellation) and constellation.is_cuda and constellation.device == dev and constellation.dtype == torch.float32
            and constellation.is_contiguous() and constellation.dim() == 2 and constellation.shape[1] == 2):
        raise ValueError("constellation must be a contiguous CUDA float32 tensor [q, 2] on %s" % dev)
    return constellation, _qam_bits(constellation.shape[0])


def _check_il(interleave):
    if interleave not in (IL_NONE, IL_ROWCOL):
        raise ValueError("interleave must be IL_NONE (0) or IL_ROWCOL (1), not %r" % (interleave,))
    return int(interleave)


def Modulate_QAM(CodeWord, N, m, F=None, device=None, stream=None, interleave=IL_NONE):
    """bldpc_qam_map_il: CodeWord CUDA int32 [N, F] (frame-fastest) -> constellation indices sym int32 [F, Ns], Ns = ceil(N / m); bit b
    of sym[f, s] is codeword bit s*m + b (IL_NONE) or b*Ns + s (IL_ROWCOL), pad bits 0 (include/bldpc.h).  CodeWord=None sends the
    all-zero word and needs F."""
    if not 1 <= int(m) <= 8:
        raise ValueError("m must be in 1..8")
    il = _check_il(interleave)
    if CodeWord is None:
        if F is None or F <= 0 or N <= 0:
            raise ValueError("CodeWord=None (the all-zero word) needs positive N and F")
        device = device or torch.device("cuda", torch.cuda.current_device())
    else:
        if not (torch.is_tensor(CodeWord) and CodeWord.dim() == 2 and CodeWord.shape[0] == N and CodeWord.shape[1] > 0):
            raise ValueError("CodeWord must be [N=%d, F]" % N)
        F, device = int(CodeWord.shape[1]), CodeWord.device
        _check_cw(CodeWord, N, F, device)
    sym = torch.empty((F, (N + m - 1) // m), dtype=torch.int32, device=device)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(device)).cuda_stream)
    check(lib.bldpc_qam_map_il(_dev_ptr(CodeWord), N, F, int(m), il, _dev_ptr(sym), st), "Modulate_QAM")
    return sym


def AWGNChannel_QAM_GPU(seed, sigma, sym, constellation, stream=None):
    """The per-frame QAM channel of the GF(q) half (nbldpc_awgn_channel_device_qam_frames) on the indices Modulate_QAM made:
    sym CUDA int32 [F, Ns], constellation CUDA float32 [q, 2] -> rx CUDA float32 [F, Ns, 2].  Four RandomModule draws per symbol;
    seed (int32[3]) is advanced by 4 * Ns * F draws."""
    if not (isinstance(seed, np.ndarray) and seed.dtype == np.int32 and seed.size == 3):
        raise ValueError("seed must be an int32 numpy array of 3")
    if not (torch.is_tensor(sym) and sym.is_cuda and sym.dtype == torch.int32 and sym.is_contiguous() and sym.dim() == 2 and sym.numel() > 0):
        raise ValueError("sym must be a contiguous CUDA int32 tensor [F, Ns]")
    con, _ = _check_con(constellation, sym.device)
    F, Ns = (int(x) for x in sym.shape)
    rx = torch.empty((F, Ns, 2), dtype=torch.float32, device=sym.device)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(sym.device)).cuda_stream)
    rc = lib.nbldpc_awgn_channel_device_qam_frames(_np_ptr(seed), ctypes.c_float(sigma), _dev_ptr(sym), Ns, _dev_ptr(con), int(con.shape[0]), F,
                                                   _dev_ptr(rx), st)
    if rc != 0:
        raise LdpcError("AWGNChannel_QAM_GPU failed (%d): %s" % (rc, lib.nbldpc_last_error().decode(errors="replace")))
    return rx


def Demodulate_QAM(rx, constellation, scale, N, stream=None, interleave=IL_NONE):
    """bldpc_qam_demap_il: max-log soft values of the N codeword bits of every frame.  rx CUDA float32 [F, Ns, 2] with
    Ns = ceil(N / log2 q), constellation CUDA float32 [q, 2] -> Channel_Out CUDA float32 [N, F] (frame-fastest, positive = bit 0),
    (m1 - m0) * scale: scale = 1 / (2 sigma^2) for LLRs, 1.0 is as good for the min-sum decoders.  interleave: the rule Modulate_QAM
    was given."""
    il = _check_il(interleave)
    if not (torch.is_tensor(rx) and rx.is_cuda and rx.dtype == torch.float32 and rx.is_contiguous() and rx.dim() == 3 and rx.shape[2] == 2):
        raise ValueError("rx must be a contiguous CUDA float32 tensor [F, Ns, 2]")
    con, m = _check_con(constellation, rx.device)
    F = int(rx.shape[0])
    if N <= 0 or F <= 0 or rx.shape[1] != (N + m - 1) // m:
        raise ValueError("rx must hold ceil(N / m) = %d symbols per frame, not %d" % ((N + m - 1) // m, rx.shape[1]))
    out = torch.empty((N, F), dtype=torch.float32, device=rx.device)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(rx.device)).cuda_stream)
    check(lib.bldpc_qam_demap_il(_dev_ptr(rx), _dev_ptr(con), int(con.shape[0]), ctypes.c_float(scale), N, F, il, _dev_ptr(out), st), "Demodulate_QAM")
    return out


def Modulate_QAM_host(CodeWord, N, m, F=None, interleave=IL_NONE):
    """bldpc_qam_map_il_host: Modulate_QAM on host arrays, no device needed (the statement of the semantics).  -> int32 [F, Ns]."""
    if not 1 <= int(m) <= 8:
        raise ValueError("m must be in 1..8")
    il = _check_il(interleave)
    if CodeWord is None:
        if F is None or F <= 0 or N <= 0:
            raise ValueError("CodeWord=None (the all-zero word) needs positive N and F")
        cw = None
    else:
        cw = np.ascontiguousarray(CodeWord, np.int32)
        if cw.ndim != 2 or cw.shape[0] != N or cw.shape[1] <= 0:
            raise ValueError("CodeWord must be [N=%d, F]" % N)
        F = cw.shape[1]
    sym = np.empty((F, (N + m - 1) // m), np.int32)
    check(lib.bldpc_qam_map_il_host(None if cw is None else _np_ptr(cw), N, F, int(m), il, _np_ptr(sym)), "Modulate_QAM_host")
    return sym


def Demodulate_QAM_host(rx, constellation, scale, N, interleave=IL_NONE):
    """bldpc_qam_demap_il_host: Demodulate_QAM on host arrays, no device needed.  rx float32 [F, Ns, 2] -> float32 [N, F]."""
    il = _check_il(interleave)
    con, m = _check_con(constellation)
    rx = np.ascontiguousarray(rx, np.float32)
    if N <= 0 or rx.ndim != 3 or rx.shape[0] <= 0 or rx.shape[1] != (N + m - 1) // m or rx.shape[2] != 2:
        raise ValueError("rx must be float32 [F, ceil(N / m) = %d, 2]" % ((N + m - 1) // m))
    F = rx.shape[0]
    out = np.empty((N, F), np.float32)
    check(lib.bldpc_qam_demap_il_host(_np_ptr(rx), _np_ptr(con), con.shape[0], ctypes.c_float(scale), N, F, il, _np_ptr(out)), "Demodulate_QAM_host")
    return out


QUASI_STATIC = 1 << 30  # a block length above every frame length: one gain per frame and transmission

_LCG_M = (61967, 63443, 63599)


class Fading:
    """Flat Rayleigh block fading with receiver CSI (include/bldpc.h, "block fading") as the sweeps take it: gains constant over blocks
    of Lc channel uses (1: fast fading; QUASI_STATIC, or anything not below the frame's channel uses: one gain per frame and
    transmission), drawn from a RandomModule stream of their own.  `seed` is kept as an int32 array of 3 that the sweeps advance in
    place like the noise seed.  A value class: check() is what the sweeps refuse it by, before anything touches the device."""

    def __init__(self, Lc, seed=(4711, 4712, 4713)):
        self.Lc = Lc
        self.seed = seed if isinstance(seed, np.ndarray) and seed.dtype == np.int32 else np.array(seed, np.int32)

    def check(self):
        if isinstance(self.Lc, bool) or not isinstance(self.Lc, (int, np.integer)) or self.Lc < 1:
            raise ValueError("fading.Lc must be an integer >= 1 (QUASI_STATIC for one gain per frame), not %r" % (self.Lc,))
        if self.seed.shape != (3,) or not all(0 <= int(self.seed[i]) < _LCG_M[i] for i in range(3)):
            raise ValueError("fading.seed must be three ints with 0 <= seed[i] < %s, not %s" % (list(_LCG_M), self.seed.tolist()))

    def __repr__(self):
        return "Fading(Lc=%r, seed=%s)" % (self.Lc, self.seed.tolist())


def _check_seed(seed):
    if not (isinstance(seed, np.ndarray) and seed.dtype == np.int32 and seed.size == 3):
        raise ValueError("seed must be an int32 numpy array of 3")


def _check_gain(gain, F, S, dev=None):
    """gain [F, S] float32: a contiguous CUDA tensor on `dev`, or (dev None) anything numpy reads."""
    if dev is None:
        g = np.ascontiguousarray(gain, np.float32)
        if g.shape != (F, S):
            raise ValueError("gain must be float32 [F=%d, S=%d], not %s" % (F, S, g.shape))
        return g
    if not (torch.is_tensor(gain) and gain.is_cuda and gain.device == dev and gain.dtype == torch.float32 and gain.is_contiguous()
            and tuple(gain.shape) == (F, S)):
        raise ValueError("gain must be a contiguous CUDA float32 tensor [F=%d, S=%d] on %s" % (F, S, dev))
    return gain


def Fading_Gains(seed, Lc, S, F, device=None, stream=None):
    """bldpc_fading_gains_device: the gains of F frames of S channel uses, constant over blocks of Lc uses, a = sqrt(-log(1 - u)) with u
    draw f * nb + j (nb = ceil(S / Lc)) of the stream at `seed` (int32[3], advanced by nb * F draws).  -> CUDA float32 [F, S]."""
    _check_seed(seed)
    if Lc < 1 or S <= 0 or F <= 0:
        raise ValueError("Fading_Gains needs Lc >= 1 and positive S and F")
    device = device or torch.device("cuda", torch.cuda.current_device())
    gain = torch.empty((F, S), dtype=torch.float32, device=device)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(device)).cuda_stream)
    check(lib.bldpc_fading_gains_device(_np_ptr(seed), int(Lc), int(S), int(F), _dev_ptr(gain), st), "Fading_Gains")
    return gain


def Fading_Gains_host(seed, Lc, S, F):
    """bldpc_fading_gains_host: Fading_Gains on the host (host libm), the statement of the semantics.  -> float32 [F, S]."""
    _check_seed(seed)
    if Lc < 1 or S <= 0 or F <= 0:
        raise ValueError("Fading_Gains_host needs Lc >= 1 and positive S and F")
    gain = np.empty((F, S), np.float32)
    check(lib.bldpc_fading_gains_host(_np_ptr(seed), int(Lc), int(S), int(F), _np_ptr(gain)), "Fading_Gains_host")
    return gain


def AWGNChannel_Fading_GPU(seed, sigma, gain, N, F, CodeWord=None, stream=None):
    """bldpc_awgn_fading_channel_device: the draws of AWGNChannel_GPU, r = a (1 - 2c) + noise, and the matched-filter value a * r as the
    decoder's input (2 / sigma^2 stays the sum-product llr_scale).  gain CUDA float32 [F, N] -> CUDA float32 [N, F]; seed advanced."""
    _check_seed(seed)
    if not torch.is_tensor(gain):
        raise ValueError("gain must be a contiguous CUDA float32 tensor [F=%d, N=%d]" % (F, N))
    _check_gain(gain, F, N, gain.device)
    if CodeWord is not None:
        _check_cw(CodeWord, N, F, gain.device)
    out = torch.empty((N, F), dtype=torch.float32, device=gain.device)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(gain.device)).cuda_stream)
    check(lib.bldpc_awgn_fading_channel_device(_np_ptr(seed), ctypes.c_float(sigma), _dev_ptr(gain), _dev_ptr(out), _dev_ptr(CodeWord), N, F, st),
          "AWGNChannel_Fading_GPU")
    return out


def AWGNChannel_Fading_CPU(seed, sigma, gain, N, F, CodeWord=None):
    """bldpc_awgn_fading_channel_host: AWGNChannel_Fading_GPU on host arrays (host libm).  -> float32 [N, F]."""
    _check_seed(seed)
    g = _check_gain(gain, F, N)
    cw = None if CodeWord is None else np.ascontiguousarray(CodeWord, np.int32)
    if cw is not None and cw.shape != (N, F):
        raise ValueError("CodeWord must be [N=%d, F=%d]" % (N, F))
    out = np.empty((N, F), np.float32)
    check(lib.bldpc_awgn_fading_channel_host(_np_ptr(seed), ctypes.c_float(sigma), _np_ptr(g), _np_ptr(out), None if cw is None else _np_ptr(cw),
                                             N, F), "AWGNChannel_Fading_CPU")
    return out


def AWGNChannel_QAM_Fading_GPU(seed, sigma, sym, constellation, gain, stream=None):
    """nbldpc_fading_channel_device_qam_frames: AWGNChannel_QAM_GPU with the point of symbol (f, s) scaled by gain[f, s] before the noise
    is added.  sym CUDA int32 [F, Ns], gain CUDA float32 [F, Ns] -> rx CUDA float32 [F, Ns, 2]; the same draws and seed advance."""
    _check_seed(seed)
    if not (torch.is_tensor(sym) and sym.is_cuda and sym.dtype == torch.int32 and sym.is_contiguous() and sym.dim() == 2 and sym.numel() > 0):
        raise ValueError("sym must be a contiguous CUDA int32 tensor [F, Ns]")
    con, _ = _check_con(constellation, sym.device)
    F, Ns = (int(x) for x in sym.shape)
    _check_gain(gain, F, Ns, sym.device)
    rx = torch.empty((F, Ns, 2), dtype=torch.float32, device=sym.device)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(sym.device)).cuda_stream)
    rc = lib.nbldpc_fading_channel_device_qam_frames(_np_ptr(seed), ctypes.c_float(sigma), _dev_ptr(sym), Ns, _dev_ptr(con), int(con.shape[0]),
                                                     _dev_ptr(gain), F, _dev_ptr(rx), st)
    if rc != 0:
        raise LdpcError("AWGNChannel_QAM_Fading_GPU failed (%d): %s" % (rc, lib.nbldpc_last_error().decode(errors="replace")))
    return rx


def AWGNChannel_QAM_Fading_CPU(seed, sigma, sym, constellation, gain):
    """nbldpc_fading_channel_host_qam_frames: AWGNChannel_QAM_Fading_GPU on host arrays (host libm).  -> float32 [F, Ns, 2]."""
    _check_seed(seed)
    sym = np.ascontiguousarray(sym, np.int32)
    if sym.ndim != 2 or sym.size == 0:
        raise ValueError("sym must be int32 [F, Ns]")
    con, _ = _check_con(constellation)
    F, Ns = sym.shape
    g = _check_gain(gain, F, Ns)
    rx = np.empty((F, Ns, 2), np.float32)
    rc = lib.nbldpc_fading_channel_host_qam_frames(_np_ptr(seed), ctypes.c_float(sigma), _np_ptr(sym), Ns, _np_ptr(con), con.shape[0], _np_ptr(g), F,
                                                   _np_ptr(rx))
    if rc != 0:
        raise LdpcError("AWGNChannel_QAM_Fading_CPU failed (%d): %s" % (rc, lib.nbldpc_last_error().decode(errors="replace")))
    return rx


def Demodulate_QAM_Fading(rx, gain, constellation, scale, N, stream=None, interleave=IL_NONE):
    """bldpc_qam_demap_fading: Demodulate_QAM with the distances taken to the faded points a * c_p, a = gain[f, s] (CUDA float32 [F, Ns],
    aligned with rx [F, Ns, 2]).  A gain of 0 gives +0.0 on all bits of its symbol (an erasure), a gain of 1 the bits of Demodulate_QAM."""
    il = _check_il(interleave)
    if not (torch.is_tensor(rx) and rx.is_cuda and rx.dtype == torch.float32 and rx.is_contiguous() and rx.dim() == 3 and rx.shape[2] == 2):
        raise ValueError("rx must be a contiguous CUDA float32 tensor [F, Ns, 2]")
    con, m = _check_con(constellation, rx.device)
    F = int(rx.shape[0])
    if N <= 0 or F <= 0 or rx.shape[1] != (N + m - 1) // m:
        raise ValueError("rx must hold ceil(N / m) = %d symbols per frame, not %d" % ((N + m - 1) // m, rx.shape[1]))
    _check_gain(gain, F, int(rx.shape[1]), rx.device)
    out = torch.empty((N, F), dtype=torch.float32, device=rx.device)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(rx.device)).cuda_stream)
    check(lib.bldpc_qam_demap_fading(_dev_ptr(rx), _dev_ptr(gain), _dev_ptr(con), int(con.shape[0]), ctypes.c_float(scale), N, F, il, _dev_ptr(out), st),
          "Demodulate_QAM_Fading")
    return out


def Demodulate_QAM_Fading_host(rx, gain, constellation, scale, N, interleave=IL_NONE):
    """bldpc_qam_demap_fading_host: Demodulate_QAM_Fading on host arrays, no device needed.  -> float32 [N, F]."""
    il = _check_il(interleave)
    con, m = _check_con(constellation)
    rx = np.ascontiguousarray(rx, np.float32)
    if N <= 0 or rx.ndim != 3 or rx.shape[0] <= 0 or rx.shape[1] != (N + m - 1) // m or rx.shape[2] != 2:
        raise ValueError("rx must be float32 [F, ceil(N / m) = %d, 2]" % ((N + m - 1) // m))
    F = rx.shape[0]
    g = _check_gain(gain, F, rx.shape[1])
    out = np.empty((N, F), np.float32)
    check(lib.bldpc_qam_demap_fading_host(_np_ptr(rx), _np_ptr(g), _np_ptr(con), con.shape[0], ctypes.c_float(scale), N, F, il, _np_ptr(out)),
          "Demodulate_QAM_Fading_host")
    return out


class RateMatch:
    """A shortening / puncturing profile over a mother code of N bits (bldpc_rm, semantics in include/bldpc.h).  shorten, puncture:
    codeword positions in [0, N), in any order, disjoint and without repeats.  E = N - n_short - n_punct bits are transmitted, in
    ascending position tx_pos (int32 [E], host).  Host only until the first device call on it.  RateMatch.circular makes the HARQ kind;
    every profile has Ncb (buffer length), k0 and laps (a linear one: E, 0, 1)."""

    def __init__(self, N, shorten=(), puncture=(), _circular=None):
        sh, pu = (np.ascontiguousarray(np.asarray(x if isinstance(x, np.ndarray) else list(x)).reshape(-1), np.int32) for x in (shorten, puncture))
        self._h = None
        h = ctypes.c_void_p()
        lists = (_np_ptr(sh) if sh.size else None, int(sh.size), _np_ptr(pu) if pu.size else None, int(pu.size))
        if _circular is None:
            check(lib.bldpc_rm_create(int(N), *lists, ctypes.byref(h)), "RateMatch")
        else:
            check(lib.bldpc_rm_create_circular(int(N), *lists, int(_circular[0]), int(_circular[1]), ctypes.byref(h)), "RateMatch.circular")
        self._h = h
        d = np.zeros(4, np.int32)
        check(lib.bldpc_rm_dims(self._h, _np_ptr(d)), "bldpc_rm_dims")
        self.N, self.E, self.n_short, self.n_punct = (int(x) for x in d)
        self.tx_pos = np.zeros(self.E, np.int32)
        check(lib.bldpc_rm_tx_pos(self._h, _np_ptr(self.tx_pos)), "bldpc_rm_tx_pos")
        self.shorten, self.puncture = np.sort(sh), np.sort(pu)
        check(lib.bldpc_rm_circ(self._h, _np_ptr(d)), "bldpc_rm_circ")
        self.Ncb, self.k0, self.laps = int(d[0]), int(d[1]), int(d[3])
        self.is_circular = _circular is not None

    @classmethod
    def circular(cls, N, shorten, puncture, k0, E):
        """bldpc_rm_create_circular: one HARQ transmission.  The buffer is the Ncb = N - n_short - n_punct positions a RateMatch of the same
        lists transmits; this profile sends tx_pos[e] = buffer[(k0 + e) % Ncb] for e < E, around the end and up to 8 times over
        (laps = ceil(E / Ncb)).  E is what rate() divides by."""
        return cls(N, shorten, puncture, _circular=(k0, E))

    def rate(self, K):
        """(K - n_short) / E: the rate of the derived code, K the information bits of the mother code."""
        return (K - self.n_short) / self.E

    def close(self):
        if self._h:
            lib.bldpc_rm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check_short_llr(short_llr):
    if not (np.isfinite(short_llr) and short_llr > 0):
        raise ValueError("short_llr must be finite and > 0, not %r" % (short_llr,))


def RM_Select(rm, CodeWord, stream=None):
    """bldpc_rm_select: CodeWord CUDA int32 [N, F] -> the transmitted rows, int32 [E, F] (tx[e] = CodeWord[tx_pos[e]])."""
    if not (torch.is_tensor(CodeWord) and CodeWord.dim() == 2 and CodeWord.shape[1] > 0):
        raise ValueError("CodeWord must be [N=%d, F]" % rm.N)
    F, dev = int(CodeWord.shape[1]), CodeWord.device
    _check_cw(CodeWord, rm.N, F, dev)
    tx = torch.empty((rm.E, F), dtype=torch.int32, device=dev)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)
    check(lib.bldpc_rm_select(rm._h, _dev_ptr(CodeWord), F, _dev_ptr(tx), st), "RM_Select")
    return tx


def RM_Recover(rm, rx, short_llr=1.0e4, stream=None):
    """bldpc_rm_recover: received values rx CUDA float32 [E, F] -> Channel_Out [N, F]: the same bits on the transmitted rows, +0.0 on
    the punctured ones, short_llr on the shortened ones."""
    if not (torch.is_tensor(rx) and rx.is_cuda and rx.dtype == torch.float32 and rx.is_contiguous() and rx.dim() == 2
            and rx.shape[0] == rm.E and rx.shape[1] > 0):
        raise ValueError("rx must be a contiguous CUDA float32 tensor [E=%d, F]" % rm.E)
    _check_short_llr(short_llr)
    F = int(rx.shape[1])
    out = torch.empty((rm.N, F), dtype=torch.float32, device=rx.device)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(rx.device)).cuda_stream)
    check(lib.bldpc_rm_recover(rm._h, _dev_ptr(rx), F, ctypes.c_float(short_llr), _dev_ptr(out), st), "RM_Recover")
    return out


def AWGNChannel_RM_GPU(rm, seed, sigma, F, device=None, CodeWord=None, short_llr=1.0e4, stream=None):
    """bldpc_rm_awgn_channel_device: the decoder's input [N, F] of a rate-matched batch from one kernel.  Noise is drawn for the E
    transmitted bits only (the rows AWGNChannel_GPU(seed, sigma, E, F, CodeWord=RM_Select(rm, CodeWord)) returns, bit for bit);
    seed (int32[3]) is advanced by 2 * E * F draws.  CodeWord: CUDA int32 [N, F] or None for the all-zero word."""
    if not (isinstance(seed, np.ndarray) and seed.dtype == np.int32 and seed.size == 3):
        raise ValueError("seed must be an int32 numpy array of 3")
    if F <= 0:
        raise ValueError("F must be positive")
    _check_short_llr(short_llr)
    device = device or torch.device("cuda", torch.cuda.current_device())
    if CodeWord is not None:
        _check_cw(CodeWord, rm.N, F, device)
    out = torch.empty((rm.N, F), dtype=torch.float32, device=device)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(device)).cuda_stream)
    check(lib.bldpc_rm_awgn_channel_device(rm._h, _np_ptr(seed), ctypes.c_float(sigma), _dev_ptr(CodeWord), F, ctypes.c_float(short_llr),
                                           _dev_ptr(out), st), "AWGNChannel_RM_GPU")
    return out


def RM_Select_host(rm, CodeWord):
    """bldpc_rm_select_host: RM_Select on a host array int32 [N, F], no device needed."""
    cw = np.ascontiguousarray(CodeWord, np.int32)
    if cw.ndim != 2 or cw.shape[0] != rm.N or cw.shape[1] <= 0:
        raise ValueError("CodeWord must be [N=%d, F]" % rm.N)
    tx = np.empty((rm.E, cw.shape[1]), np.int32)
    check(lib.bldpc_rm_select_host(rm._h, _np_ptr(cw), cw.shape[1], _np_ptr(tx)), "RM_Select_host")
    return tx


def RM_Recover_host(rm, rx, short_llr=1.0e4):
    """bldpc_rm_recover_host: RM_Recover on a host array float32 [E, F], no device needed."""
    rx = np.ascontiguousarray(rx, np.float32)
    if rx.ndim != 2 or rx.shape[0] != rm.E or rx.shape[1] <= 0:
        raise ValueError("rx must be [E=%d, F]" % rm.E)
    out = np.empty((rm.N, rx.shape[1]), np.float32)
    check(lib.bldpc_rm_recover_host(rm._h, _np_ptr(rx), rx.shape[1], ctypes.c_float(short_llr), _np_ptr(out)), "RM_Recover_host")
    return out


def RM_Select_Bits(rm, bits, F, stream=None):
    """bldpc_rm_select_bits: packed words CUDA int32 [N, ceil(F/32)] -> the transmitted rows [E, ceil(F/32)] (tx[e] = bits[tx_pos[e]]),
    padding written as 0: Hard_Pack_Int(RM_Select(rm, .)) of the unpacked words, bit for bit."""
    if not (torch.is_tensor(bits) and bits.is_cuda):
        raise ValueError("bits must be a CUDA int32 tensor [N=%d, ceil(F/32)]" % rm.N)
    _check_bits(bits, rm.N, F, bits.device)
    tx = torch.empty((rm.E, _words(F)), dtype=torch.int32, device=bits.device)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(bits.device)).cuda_stream)
    check(lib.bldpc_rm_select_bits(rm._h, _dev_ptr(bits), int(F), _dev_ptr(tx), st), "RM_Select_Bits")
    return tx


def RM_Recover_Bits(rm, rx_bits, F, rx_erased=None, stream=None):
    """bldpc_rm_recover_bits: received packed words [E, ceil(F/32)] and their erasure mask (None: nothing erased) -> (bits, erased) of
    the mother code, CUDA int32 [N, ceil(F/32)]: shortened positions known 0, punctured and unsent ones erased, a position sent several
    times takes its first unerased copy."""
    if not (torch.is_tensor(rx_bits) and rx_bits.is_cuda):
        raise ValueError("rx_bits must be a CUDA int32 tensor [E=%d, ceil(F/32)]" % rm.E)
    dev = rx_bits.device
    _check_bits(rx_bits, rm.E, F, dev)
    if rx_erased is not None:
        if not (torch.is_tensor(rx_erased) and rx_erased.is_cuda and rx_erased.device == dev):
            raise ValueError("rx_erased must be a CUDA int32 tensor [E=%d, ceil(F/32)] on %s" % (rm.E, dev))
        _check_bits(rx_erased, rm.E, F, dev)
    bits = torch.empty((rm.N, _words(F)), dtype=torch.int32, device=dev)
    erased = torch.empty((rm.N, _words(F)), dtype=torch.int32, device=dev)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)
    check(lib.bldpc_rm_recover_bits(rm._h, _dev_ptr(rx_bits), _dev_ptr(rx_erased), int(F), _dev_ptr(bits), _dev_ptr(erased), st), "RM_Recover_Bits")
    return bits, erased


def RM_Select_Bits_host(rm, bits, F):
    """bldpc_rm_select_bits_host: RM_Select_Bits on a host array uint32 [N, ceil(F/32)], no device needed."""
    bits = _check_bits(bits, rm.N, F)
    tx = np.empty((rm.E, _words(F)), np.uint32)
    check(lib.bldpc_rm_select_bits_host(rm._h, _np_ptr(bits), int(F), _np_ptr(tx)), "RM_Select_Bits_host")
    return tx


def RM_Recover_Bits_host(rm, rx_bits, F, rx_erased=None):
    """bldpc_rm_recover_bits_host: RM_Recover_Bits on host arrays uint32 [E, ceil(F/32)], no device needed.  Returns (bits, erased)."""
    rx_bits = _check_bits(rx_bits, rm.E, F)
    rx_erased = None if rx_erased is None else _check_bits(rx_erased, rm.E, F)
    bits, erased = np.empty((rm.N, _words(F)), np.uint32), np.empty((rm.N, _words(F)), np.uint32)
    check(lib.bldpc_rm_recover_bits_host(rm._h, _np_ptr(rx_bits), None if rx_erased is None else _np_ptr(rx_erased), int(F), _np_ptr(bits),
                                         _np_ptr(erased)), "RM_Recover_Bits_host")
    return bits, erased


def AWGNChannel_RM_CPU(rm, seed, sigma, F, CodeWord=None, short_llr=1.0e4):
    """bldpc_rm_awgn_channel_host: RM_Recover_host(AWGNChannel_CPU(seed, sigma, E, F, CodeWord=CodeWord[tx_pos])) in one call, host
    libm; seed (int32[3]) advanced by 2 * E * F draws.  Returns float32 [N, F]."""
    if not (isinstance(seed, np.ndarray) and seed.dtype == np.int32 and seed.size == 3):
        raise ValueError("seed must be an int32 numpy array of 3")
    cw = None
    if CodeWord is not None:
        cw = np.ascontiguousarray(CodeWord, np.int32)
        if cw.shape != (rm.N, F):
            raise ValueError("CodeWord must be [N=%d, F=%d]" % (rm.N, F))
    out = np.empty((rm.N, F), np.float32)
    check(lib.bldpc_rm_awgn_channel_host(rm._h, _np_ptr(seed), ctypes.c_float(sigma), None if cw is None else _np_ptr(cw), int(F),
                                         ctypes.c_float(short_llr), _np_ptr(out)), "AWGNChannel_RM_CPU")
    return out


def _check_done(done, F, dev):
    if done is not None and not (torch.is_tensor(done) and done.is_cuda and done.device == dev and done.dtype == torch.int32 and done.dim() == 1
                                 and done.is_contiguous() and done.shape[0] == F):
        raise ValueError("done must be a contiguous CUDA int32 tensor [F=%d] on %s (a row of D will do)" % (F, dev))


def _check_acc(rm, Channel_Acc):
    if not (torch.is_tensor(Channel_Acc) and Channel_Acc.is_cuda and Channel_Acc.dtype == torch.float32 and Channel_Acc.is_contiguous()
            and Channel_Acc.dim() == 2 and Channel_Acc.shape[0] == rm.N and Channel_Acc.shape[1] > 0):
        raise ValueError("Channel_Acc must be a contiguous CUDA float32 tensor [N=%d, F]" % rm.N)


def RM_Combine(rm, rx, Channel_Acc, done=None, short_llr=1.0e4, stream=None):
    """bldpc_rm_combine: add one more transmission rx CUDA float32 [E, F] into Channel_Acc [N, F] in place (and return it): every
    position's contributions in ascending e, starting from the stored value; shortened rows are set to short_llr; rows without a
    contribution and the columns of frames with done[f] != 0 (CUDA int32 [F], e.g. D[N]) keep their bits."""
    _check_acc(rm, Channel_Acc)
    F, dev = int(Channel_Acc.shape[1]), Channel_Acc.device
    if not (torch.is_tensor(rx) and rx.is_cuda and rx.device == dev and rx.dtype == torch.float32 and rx.is_contiguous()
            and tuple(rx.shape) == (rm.E, F)):
        raise ValueError("rx must be a contiguous CUDA float32 tensor [E=%d, F=%d]" % (rm.E, F))
    _check_short_llr(short_llr)
    _check_done(done, F, dev)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)
    check(lib.bldpc_rm_combine(rm._h, _dev_ptr(rx), F, ctypes.c_float(short_llr), _dev_ptr(done), _dev_ptr(Channel_Acc), st), "RM_Combine")
    return Channel_Acc


def AWGNChannel_RM_Combine_GPU(rm, seed, sigma, Channel_Acc, done=None, CodeWord=None, short_llr=1.0e4, stream=None):
    """bldpc_rm_awgn_combine_device: the samples AWGNChannel_RM_GPU would draw for this transmission, combined into Channel_Acc [N, F] in
    place under done, from one kernel.  seed (int32[3]) is advanced by 2 * E * F draws whatever done holds."""
    if not (isinstance(seed, np.ndarray) and seed.dtype == np.int32 and seed.size == 3):
        raise ValueError("seed must be an int32 numpy array of 3")
    _check_acc(rm, Channel_Acc)
    F, dev = int(Channel_Acc.shape[1]), Channel_Acc.device
    _check_short_llr(short_llr)
    _check_done(done, F, dev)
    if CodeWord is not None:
        _check_cw(CodeWord, rm.N, F, dev)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)
    check(lib.bldpc_rm_awgn_combine_device(rm._h, _np_ptr(seed), ctypes.c_float(sigma), _dev_ptr(CodeWord), F, ctypes.c_float(short_llr),
                                           _dev_ptr(done), _dev_ptr(Channel_Acc), st), "AWGNChannel_RM_Combine_GPU")
    return Channel_Acc


def _host_acc(rm, acc):
    if not (isinstance(acc, np.ndarray) and acc.dtype == np.float32 and acc.flags.c_contiguous and acc.ndim == 2 and acc.shape[0] == rm.N
            and acc.shape[1] > 0):
        raise ValueError("Channel_Acc must be a C-contiguous float32 array [N=%d, F], updated in place" % rm.N)
    return acc, acc.shape[1]


def _host_done(done, F):
    if done is None:
        return None
    done = np.ascontiguousarray(done, np.int32)
    if done.shape != (F,):
        raise ValueError("done must be int32 [F=%d]" % F)
    return done


def RM_Combine_host(rm, rx, Channel_Acc, done=None, short_llr=1.0e4):
    """bldpc_rm_combine_host: RM_Combine on host arrays, no device needed.  Channel_Acc float32 [N, F] (C-contiguous) is updated in place."""
    acc, F = _host_acc(rm, Channel_Acc)
    rx = np.ascontiguousarray(rx, np.float32)
    if rx.shape != (rm.E, F):
        raise ValueError("rx must be [E=%d, F=%d]" % (rm.E, F))
    done = _host_done(done, F)
    check(lib.bldpc_rm_combine_host(rm._h, _np_ptr(rx), F, ctypes.c_float(short_llr), None if done is None else _np_ptr(done), _np_ptr(acc)),
          "RM_Combine_host")
    return acc


def AWGNChannel_RM_Combine_CPU(rm, seed, sigma, Channel_Acc, done=None, CodeWord=None, short_llr=1.0e4):
    """bldpc_rm_awgn_combine_host: RM_Select_host, AWGNChannel_CPU at E, RM_Combine_host in one call; seed advanced by 2 * E * F draws."""
    if not (isinstance(seed, np.ndarray) and seed.dtype == np.int32 and seed.size == 3):
        raise ValueError("seed must be an int32 numpy array of 3")
    acc, F = _host_acc(rm, Channel_Acc)
    cw = None
    if CodeWord is not None:
        cw = np.ascontiguousarray(CodeWord, np.int32)
        if cw.shape != (rm.N, F):
            raise ValueError("CodeWord must be [N=%d, F=%d]" % (rm.N, F))
    done = _host_done(done, F)
    check(lib.bldpc_rm_awgn_combine_host(rm._h, _np_ptr(seed), ctypes.c_float(sigma), None if cw is None else _np_ptr(cw), F,
                                         ctypes.c_float(short_llr), None if done is None else _np_ptr(done), _np_ptr(acc)), "AWGNChannel_RM_Combine_CPU")
    return acc

# ---- rate matching over QAM: the fused calls (include/bldpc.h, "rate matching over QAM") ----
def _check_rm_rx(rm, rx, m, dev=None):
    """rx [F, ceil(E / m), 2] float32: a contiguous CUDA tensor (dev: True), or anything numpy reads.  Returns (rx, F)."""
    Ns = (rm.E + m - 1) // m
    if dev:
        if not (torch.is_tensor(rx) and rx.is_cuda and rx.dtype == torch.float32 and rx.is_contiguous() and rx.dim() == 3
                and rx.shape[0] > 0 and rx.shape[1] == Ns and rx.shape[2] == 2):
            raise ValueError("rx must be a contiguous CUDA float32 tensor [F, ceil(E / m) = %d, 2]" % Ns)
    else:
        rx = np.ascontiguousarray(rx, np.float32)
        if rx.ndim != 3 or rx.shape[0] <= 0 or rx.shape[1] != Ns or rx.shape[2] != 2:
            raise ValueError("rx must be float32 [F, ceil(E / m) = %d, 2]" % Ns)
    return rx, int(rx.shape[0])


def RM_Modulate_QAM(rm, CodeWord, m, F=None, device=None, stream=None, interleave=IL_NONE):
    """bldpc_rm_qam_map: Modulate_QAM(RM_Select(rm, CodeWord), rm.E, m, interleave=...) in one pass, no [E, F] array.  CodeWord CUDA
    int32 [N, F] -> sym int32 [F, ceil(E / m)].  CodeWord=None sends the all-zero word and needs F."""
    if not 1 <= int(m) <= 8:
        raise ValueError("m must be in 1..8")
    il = _check_il(interleave)
    if CodeWord is None:
        if F is None or F <= 0:
            raise ValueError("CodeWord=None (the all-zero word) needs a positive F")
        device = device or torch.device("cuda", torch.cuda.current_device())
    else:
        if not (torch.is_tensor(CodeWord) and CodeWord.dim() == 2 and CodeWord.shape[0] == rm.N and CodeWord.shape[1] > 0):
            raise ValueError("CodeWord must be [N=%d, F]" % rm.N)
        F, device = int(CodeWord.shape[1]), CodeWord.device
        _check_cw(CodeWord, rm.N, F, device)
    sym = torch.empty((F, (rm.E + m - 1) // m), dtype=torch.int32, device=device)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(device)).cuda_stream)
    check(lib.bldpc_rm_qam_map(rm._h, _dev_ptr(CodeWord), F, int(m), il, _dev_ptr(sym), st), "RM_Modulate_QAM")
    return sym


def RM_Demodulate_QAM_Recover(rm, rx, constellation, scale, short_llr=1.0e4, stream=None, interleave=IL_NONE):
    """bldpc_rm_qam_recover: RM_Recover(rm, Demodulate_QAM(rx, constellation, scale, rm.E, interleave=...), short_llr) in one pass.
    rx CUDA float32 [F, ceil(E / m), 2] -> Channel_Out [N, F]."""
    il = _check_il(interleave)
    _check_short_llr(short_llr)
    if not (torch.is_tensor(rx) and rx.is_cuda):
        raise ValueError("rx must be a contiguous CUDA float32 tensor [F, Ns, 2]")
    con, m = _check_con(constellation, rx.device)
    rx, F = _check_rm_rx(rm, rx, m, dev=True)
    out = torch.empty((rm.N, F), dtype=torch.float32, device=rx.device)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(rx.device)).cuda_stream)
    check(lib.bldpc_rm_qam_recover(rm._h, _dev_ptr(rx), _dev_ptr(con), int(con.shape[0]), ctypes.c_float(scale), il, F, ctypes.c_float(short_llr),
                                   _dev_ptr(out), st), "RM_Demodulate_QAM_Recover")
    return out


def RM_Demodulate_QAM_Combine(rm, rx, constellation, scale, Channel_Acc, done=None, short_llr=1.0e4, stream=None, interleave=IL_NONE):
    """bldpc_rm_qam_combine: RM_Combine(rm, Demodulate_QAM(rx, constellation, scale, rm.E, interleave=...), Channel_Acc, done, short_llr)
    in one pass: Channel_Acc [N, F] is updated in place and returned; the columns of frames with done[f] != 0 keep their bits."""
    il = _check_il(interleave)
    _check_short_llr(short_llr)
    _check_acc(rm, Channel_Acc)
    F, dev = int(Channel_Acc.shape[1]), Channel_Acc.device
    con, m = _check_con(constellation, dev)
    rx, Frx = _check_rm_rx(rm, rx, m, dev=True)
    if Frx != F or rx.device != dev:
        raise ValueError("rx holds %d frames, Channel_Acc %d (both on %s)" % (Frx, F, dev))
    _check_done(done, F, dev)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)
    check(lib.bldpc_rm_qam_combine(rm._h, _dev_ptr(rx), _dev_ptr(con), int(con.shape[0]), ctypes.c_float(scale), il, F, ctypes.c_float(short_llr),
                                   _dev_ptr(done), _dev_ptr(Channel_Acc), st), "RM_Demodulate_QAM_Combine")
    return Channel_Acc


def RM_Modulate_QAM_host(rm, CodeWord, m, F=None, interleave=IL_NONE):
    """bldpc_rm_qam_map_host: RM_Modulate_QAM on host arrays, no device needed.  -> int32 [F, ceil(E / m)]."""
    if not 1 <= int(m) <= 8:
        raise ValueError("m must be in 1..8")
    il = _check_il(interleave)
    if CodeWord is None:
        if F is None or F <= 0:
            raise ValueError("CodeWord=None (the all-zero word) needs a positive F")
        cw = None
    else:
        cw = np.ascontiguousarray(CodeWord, np.int32)
        if cw.ndim != 2 or cw.shape[0] != rm.N or cw.shape[1] <= 0:
            raise ValueError("CodeWord must be [N=%d, F]" % rm.N)
        F = cw.shape[1]
    sym = np.empty((F, (rm.E + m - 1) // m), np.int32)
    check(lib.bldpc_rm_qam_map_host(rm._h, None if cw is None else _np_ptr(cw), F, int(m), il, _np_ptr(sym)), "RM_Modulate_QAM_host")
    return sym


def RM_Demodulate_QAM_Recover_host(rm, rx, constellation, scale, short_llr=1.0e4, interleave=IL_NONE):
    """bldpc_rm_qam_recover_host: RM_Demodulate_QAM_Recover on host arrays, no device needed.  -> float32 [N, F]."""
    il = _check_il(interleave)
    con, m = _check_con(constellation)
    rx, F = _check_rm_rx(rm, rx, m)
    out = np.empty((rm.N, F), np.float32)
    check(lib.bldpc_rm_qam_recover_host(rm._h, _np_ptr(rx), _np_ptr(con), con.shape[0], ctypes.c_float(scale), il, F, ctypes.c_float(short_llr),
                                        _np_ptr(out)), "RM_Demodulate_QAM_Recover_host")
    return out


def RM_Demodulate_QAM_Combine_host(rm, rx, constellation, scale, Channel_Acc, done=None, short_llr=1.0e4, interleave=IL_NONE):
    """bldpc_rm_qam_combine_host: RM_Demodulate_QAM_Combine on host arrays; Channel_Acc float32 [N, F] (C-contiguous) is updated in place."""
    il = _check_il(interleave)
    acc, F = _host_acc(rm, Channel_Acc)
    con, m = _check_con(constellation)
    rx, Frx = _check_rm_rx(rm, rx, m)
    if Frx != F:
        raise ValueError("rx holds %d frames, Channel_Acc %d" % (Frx, F))
    done = _host_done(done, F)
    check(lib.bldpc_rm_qam_combine_host(rm._h, _np_ptr(rx), _np_ptr(con), con.shape[0], ctypes.c_float(scale), il, F, ctypes.c_float(short_llr),
                                        None if done is None else _np_ptr(done), _np_ptr(acc)), "RM_Demodulate_QAM_Combine_host")
    return acc


def _check_frames_dev(src, idx, what):
    if not (torch.is_tensor(src) and src.is_cuda and src.is_contiguous() and src.element_size() == 4 and src.dim() in (1, 2) and src.numel() > 0):
        raise ValueError("%s must be a contiguous CUDA tensor of 32-bit elements, [rows, F] or [F]" % what)
    if not (torch.is_tensor(idx) and idx.is_cuda and idx.device == src.device and idx.dtype == torch.int32 and idx.is_contiguous() and idx.dim() == 1
            and idx.numel() > 0):
        raise ValueError("idx must be a non-empty contiguous CUDA int32 tensor [Fa] on the device of %s" % what)


def Frames_Gather(src, idx, stream=None):
    """bldpc_frames_gather: the columns idx (CUDA int32 [Fa], strictly ascending in [0, F)) of src, a CUDA tensor [rows, F] or [F] of
    32-bit elements -> [rows, Fa] or [Fa] of the same dtype."""
    _check_frames_dev(src, idx, "src")
    F, Fa = int(src.shape[-1]), int(idx.numel())
    if Fa > F:
        raise ValueError("idx holds %d frames, src has %d" % (Fa, F))
    dst = torch.empty(tuple(src.shape[:-1]) + (Fa,), dtype=src.dtype, device=src.device)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(src.device)).cuda_stream)
    check(lib.bldpc_frames_gather(_dev_ptr(src), src.numel() // F, F, _dev_ptr(idx), Fa, _dev_ptr(dst), st), "Frames_Gather")
    return dst


def Frames_Scatter(src, idx, dst, stream=None):
    """bldpc_frames_scatter: dst[:, idx[a]] = src[:, a] in place (and returns dst); src [rows, Fa] or [Fa], dst [rows, F] or [F], the
    other columns of dst keep their bits."""
    _check_frames_dev(src, idx, "src")
    if not (torch.is_tensor(dst) and dst.is_cuda and dst.device == src.device and dst.is_contiguous() and dst.dtype == src.dtype
            and dst.dim() == src.dim() and dst.shape[:-1] == src.shape[:-1]):
        raise ValueError("dst must be a contiguous CUDA tensor like src with F columns")
    F, Fa = int(dst.shape[-1]), int(idx.numel())
    if int(src.shape[-1]) != Fa or Fa > F:
        raise ValueError("src holds %d frames, idx %d, dst %d" % (src.shape[-1], Fa, F))
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(src.device)).cuda_stream)
    check(lib.bldpc_frames_scatter(_dev_ptr(src), src.numel() // Fa, F, _dev_ptr(idx), Fa, _dev_ptr(dst), st), "Frames_Scatter")
    return dst


def _frames_host(src, idx):
    src = np.ascontiguousarray(src)
    if src.dtype.itemsize != 4 or src.ndim not in (1, 2) or src.size == 0:
        raise ValueError("src must hold 32-bit elements, [rows, F] or [F]")
    return src, np.ascontiguousarray(idx, np.int32).reshape(-1)


def Frames_Gather_host(src, idx):
    """bldpc_frames_gather_host: Frames_Gather on host arrays; idx is checked (strictly ascending in [0, F))."""
    src, idx = _frames_host(src, idx)
    F = src.shape[-1]
    dst = np.empty(src.shape[:-1] + (idx.size,), src.dtype)
    check(lib.bldpc_frames_gather_host(_np_ptr(src), src.size // F, F, _np_ptr(idx), int(idx.size), _np_ptr(dst)), "Frames_Gather_host")
    return dst


def Frames_Scatter_host(src, idx, dst):
    """bldpc_frames_scatter_host: Frames_Scatter on host arrays, dst (C-contiguous, same dtype) updated in place."""
    src, idx = _frames_host(src, idx)
    if not (isinstance(dst, np.ndarray) and dst.flags.c_contiguous and dst.dtype == src.dtype and dst.ndim == src.ndim
            and dst.shape[:-1] == src.shape[:-1]) or src.shape[-1] != idx.size:
        raise ValueError("dst must be a C-contiguous array like src with F columns, src must hold one column per index")
    F = dst.shape[-1]
    check(lib.bldpc_frames_scatter_host(_np_ptr(src), src.size // max(idx.size, 1), F, _np_ptr(idx), int(idx.size), _np_ptr(dst)), "Frames_Scatter_host")
    return dst


def Decode_Statistic(code, Channel_Out, counters, max_iter=50, length=0, exit_mode=EXIT_BATCH_GLOBAL, kernel=KERNEL_AUTO, D=None, stream=None):
    """LDPC_Decoder_GPU followed by Statistic against the all-zero codeword, the pair of calls of Simulation_GPU's loop
    (Simulation.cu:143-145), as ONE call of the C ABI (bldpc_decode_statistic): same D, same iteration counts, same counters
    (device int64[5], accumulated); with a single-launch exit mode the errors are counted while D is written.
    Returns dict(D, iteraTime or None, iters or None)."""
    if not (Channel_Out.is_cuda and Channel_Out.dtype == torch.float32 and Channel_Out.is_contiguous()):
        raise ValueError("Channel_Out must be a contiguous CUDA float32 tensor")
    if Channel_Out.dim() != 2 or Channel_Out.shape[0] != code.N:
        raise ValueError("Channel_Out must be [N=%d, F]" % code.N)
    F = int(Channel_Out.shape[1])
    dev = Channel_Out.device
    _check_counters(counters, 5, dev)
    if D is None:
        D = torch.empty((code.N + 1, F), dtype=torch.int32, device=dev)
    else:
        _check_D(D, code.N, F, dev)
    iters = torch.empty(F, dtype=torch.int32, device=dev) if exit_mode == EXIT_PER_FRAME else None
    it = ctypes.c_int(0)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)
    check(lib.bldpc_decode_statistic(code._h, _dev_ptr(Channel_Out), F, max_iter, length, exit_mode, kernel, _dev_ptr(D), _dev_ptr(iters),
                                     _dev_ptr(counters), ctypes.byref(it), st), "Decode_Statistic")
    return dict(D=D, iteraTime=None if iters is not None else it.value, iters=iters)


@dataclass
class SimCounters:
    """The counters of struct Simulation (struct.cuh:17-33)."""
    num_Frames: int = 0
    num_Error_Frames: int = 0
    num_Error_Bits: int = 0
    Total_Iteration: int = 0
    num_False_Frames: int = 0
    num_Alarm_Frames: int = 0
    SNR: float = 0.0
    _dev: object = field(default=None, repr=False)
    num_OSD_Frames: int = field(default=0, repr=False, compare=False)   # Simulation_GPU(osd=True): frames reprocessed, and those of
    num_OSD_Correct: int = field(default=0, repr=False, compare=False)  # them that came out equal to the word sent

    def ratios(self, length):
        n = max(self.num_Frames, 1)
        return dict(FER=self.num_Error_Frames / n, BER=self.num_Error_Bits / n / length, AverageIT=self.Total_Iteration / n,
                    FER_False=self.num_False_Frames / n, FER_Alarm=self.num_Alarm_Frames / n)


def Statistic(SIM, code, D, iteraTime, length=0, CodeWord=None, leastErrorFrames=50, leastTestFrames=10000, stream=None):
    """Statistic (Simulation.cu:245-285) on the device; returns the reference's stop flag.

    The caller adds the batch to SIM.num_Frames first, like Simulation_GPU does (Simulation.cu:113).
    iteraTime: the batch's iteration count (int), or the per-frame counts of EXIT_PER_FRAME (CUDA int32 tensor [F])."""
    F = int(D.shape[1])
    if SIM._dev is None:
        SIM._dev = torch.zeros(5, dtype=torch.int64, device=D.device)
    st = ctypes.c_void_p((stream or torch.cuda.current_stream(D.device)).cuda_stream)
    if torch.is_tensor(iteraTime):
        check(lib.bldpc_statistic_per_frame(code._h, _dev_ptr(D), _dev_ptr(CodeWord), F, length, _dev_ptr(iteraTime), _dev_ptr(SIM._dev), st),
              "Statistic")
    else:
        check(lib.bldpc_statistic(code._h, _dev_ptr(D), _dev_ptr(CodeWord), F, length, iteraTime, _dev_ptr(SIM._dev), st), "Statistic")
    c = SIM._dev.cpu().tolist()
    SIM.num_Error_Frames, SIM.num_Error_Bits, SIM.Total_Iteration, SIM.num_False_Frames, SIM.num_Alarm_Frames = c
    return 1 if (SIM.num_Error_Frames >= leastErrorFrames and SIM.num_Frames >= leastTestFrames) else 0
