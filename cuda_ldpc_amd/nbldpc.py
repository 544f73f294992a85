"""Host-side mirror of the reference's non-binary LDPC entry points (myNBLDPC/).

Same names and argument meaning as src/Simulation.cpp, src/GF.cpp, src/LDPC_Decoder.cpp and
src/LDPC_Encoder.cpp; the `define.h` macros (GFQ, maxdc, EMS_NM, EMS_NC, maxIT) become arguments.
All computation goes through the C ABI of include/nbldpc.h; tensors are torch CUDA(HIP) tensors.
"""
import ctypes

import numpy as np
import torch

from ._lib import LdpcError, lib

c_int, c_void_p, c_char_p, c_float = ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_float

lib.nbldpc_last_error.restype = c_char_p
lib.nbldpc_read_matrix.argtypes = [c_char_p] + [c_void_p] * 7
lib.nbldpc_gf_load.argtypes = [c_char_p, c_int, c_void_p, c_void_p, c_void_p]
lib.nbldpc_gf_generate.argtypes = [c_int, ctypes.c_uint, c_void_p, c_void_p, c_void_p]
lib.nbldpc_code_create.argtypes = [c_int] * 5 + [c_void_p] * 7 + [ctypes.POINTER(c_void_p)]
lib.nbldpc_code_destroy.argtypes = [c_void_p]
lib.nbldpc_ems_decode_batch.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int] + [c_void_p] * 6
lib.nbldpc_tmm_decode_batch.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int] + [c_void_p] * 6
lib.nbldpc_qspa_decode_batch.argtypes = [c_void_p, c_void_p, c_int, c_int] + [c_void_p] * 6
lib.nbldpc_qspa_decode_host.argtypes = [c_int] * 5 + [c_void_p] * 8 + [c_int, c_int] + [c_void_p] * 5
lib.nbldpc_qspa_exp_host.argtypes = [c_void_p, c_int, c_void_p]
lib.nbldpc_qspa_layered_decode_batch.argtypes = lib.nbldpc_qspa_decode_batch.argtypes
lib.nbldpc_qspa_layered_decode_host.argtypes = lib.nbldpc_qspa_decode_host.argtypes
lib.nbldpc_qspa_layered_threads.argtypes = [c_void_p]
lib.nbldpc_qspa_ws_decode_batch.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int] + [c_void_p] * 6
lib.nbldpc_qspa_ws_plan_host.argtypes = [c_int] * 6 + [c_void_p]
lib.nbldpc_qspa_ws_info.argtypes = [c_void_p, c_int, c_void_p]
lib.nbldpc_qspa_ws_slots.argtypes = [c_void_p, c_int, c_int]
lib.nbldpc_demodulate_bpsk.argtypes = [c_void_p, c_void_p, c_float, c_int, c_void_p, c_void_p]
lib.nbldpc_statistic.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]
lib.nbldpc_awgn_channel_host.argtypes = [c_void_p, c_float, c_void_p, c_int, c_int, c_void_p]
lib.nbldpc_awgn_channel_device.argtypes = [c_void_p, c_float, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]
lib.nbldpc_read_constellation.argtypes = [c_char_p, c_int, c_void_p]
lib.nbldpc_last_kernel.argtypes = [c_void_p]
lib.nbldpc_last_kernel.restype = ctypes.c_char_p
lib.nbldpc_code_grids.argtypes = [c_void_p, c_void_p]
lib.nbldpc_awgn_channel_host_qam.argtypes = [c_void_p, c_float, c_void_p, c_int, c_void_p, c_int, c_void_p]
lib.nbldpc_awgn_channel_device_qam.argtypes = [c_void_p, c_float, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]
lib.nbldpc_demodulate_qam.argtypes = [c_void_p, c_void_p, c_void_p, c_float, c_int, c_void_p, c_void_p]
lib.nbldpc_sigma.restype = c_float
lib.nbldpc_sigma.argtypes = [c_float, c_int, c_int, c_float]
lib.nbldpc_generator_host.argtypes = [c_int] * 4 + [c_void_p] * 4 + [ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_void_p, c_void_p]
lib.nbldpc_encoder_info.argtypes = [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_void_p]
lib.nbldpc_encode.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p]
lib.nbldpc_encode_random.argtypes = [c_void_p, ctypes.c_ulonglong, ctypes.c_longlong, c_int, c_void_p, c_void_p, c_void_p]
lib.nbldpc_syndrome.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]
lib.nbldpc_awgn_channel_device_frames.argtypes = [c_void_p, c_float, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]
lib.nbldpc_awgn_channel_device_qam_frames.argtypes = [c_void_p, c_float, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p]
lib.nbldpc_statistic_frames.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]
lib.nbldpc_demodulate_bpsk_nq.argtypes = [c_int, c_int, c_void_p, c_float, c_int, c_void_p, c_void_p]
lib.nbldpc_demodulate_qam_nq.argtypes = [c_int, c_int, c_void_p, c_void_p, c_float, c_int, c_void_p, c_void_p]
lib.nbldpc_demodulate_bpsk_nq_host.argtypes = [c_int, c_int, c_void_p, c_float, c_int, c_void_p]
lib.nbldpc_demodulate_qam_nq_host.argtypes = [c_int, c_int, c_void_p, c_void_p, c_float, c_int, c_void_p]
lib.nbldpc_rm_select.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p]
lib.nbldpc_rm_recover.argtypes = [c_void_p, c_int, c_void_p, c_int, c_float, c_void_p, c_void_p]
lib.nbldpc_rm_combine.argtypes = [c_void_p, c_int, c_void_p, c_int, c_float, c_void_p, c_void_p, c_void_p]
lib.nbldpc_rm_demodulate_qam_recover.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_float, c_int, c_float, c_void_p, c_void_p]
lib.nbldpc_rm_demodulate_qam_combine.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_float, c_int, c_float, c_void_p, c_void_p, c_void_p]
lib.nbldpc_rm_demodulate_bpsk_recover.argtypes = [c_void_p, c_int, c_void_p, c_float, c_int, c_float, c_void_p, c_void_p]
lib.nbldpc_rm_demodulate_bpsk_combine.argtypes = [c_void_p, c_int, c_void_p, c_float, c_int, c_float, c_void_p, c_void_p, c_void_p]
lib.nbldpc_rm_encode_random.argtypes = [c_void_p, c_void_p, ctypes.c_ulonglong, ctypes.c_longlong, c_int, c_void_p, c_void_p, c_void_p]
lib.nbldpc_rm_select_host.argtypes = [c_void_p, c_void_p, c_int, c_void_p]
lib.nbldpc_rm_recover_host.argtypes = [c_void_p, c_int, c_void_p, c_int, c_float, c_void_p]
lib.nbldpc_rm_combine_host.argtypes = [c_void_p, c_int, c_void_p, c_int, c_float, c_void_p, c_void_p]
lib.nbldpc_rm_demodulate_qam_recover_host.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_float, c_int, c_float, c_void_p]
lib.nbldpc_rm_demodulate_qam_combine_host.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_float, c_int, c_float, c_void_p, c_void_p]
lib.nbldpc_rm_demodulate_bpsk_recover_host.argtypes = [c_void_p, c_int, c_void_p, c_float, c_int, c_float, c_void_p]
lib.nbldpc_rm_demodulate_bpsk_combine_host.argtypes = [c_void_p, c_int, c_void_p, c_float, c_int, c_float, c_void_p, c_void_p]
lib.nbldpc_rm_force_shortened_host.argtypes = [c_void_p, c_void_p, c_int, c_int, c_void_p]


def _check(rc, what):
    if rc != 0:
        raise LdpcError("%s failed (%d): %s" % (what, rc, lib.nbldpc_last_error().decode(errors="replace")))


def _np(a):
    return a.ctypes.data_as(c_void_p)


def _dev(t):
    return None if t is None else c_void_p(t.data_ptr())


def GFInitial(q, path=None, primitive_poly=None):
    """GFInitial (GF.cpp:68-117) -> (TableMultiply[q,q], TableAdd[q,q], TableInverse[q]) uint32 host arrays.
    Either read the reference's table file or generate from the primitive polynomial."""
    mul = np.zeros((q, q), np.uint32)
    add = np.zeros((q, q), np.uint32)
    inv = np.zeros(q, np.uint32)
    if path is not None:
        _check(lib.nbldpc_gf_load(str(path).encode(), q, _np(mul), _np(add), _np(inv)), "GFInitial")
    else:
        _check(lib.nbldpc_gf_generate(q, primitive_poly, _np(mul), _np(add), _np(inv)), "GFInitial(generate)")
    return mul, add, inv


class NBMatrix:
    """Get_H (Simulation.cpp:347-467) on the host only: N, M, q, dv, dc, rate and the flattened VN/CN arrays."""

    def __init__(self, matrix_path):
        dims = np.zeros(5, np.int32)
        _check(lib.nbldpc_read_matrix(str(matrix_path).encode(), _np(dims), None, None, None, None, None, None), "Get_H")
        self.N, self.M, self.q, self.dv, self.dc = (int(x) for x in dims)
        self.m = int(np.log2(self.q))
        self.vn_weight = np.zeros(self.N, np.int32)
        self.vn_linkCNs = np.zeros((self.N, self.dv), np.int32)
        self.vn_linkCNs_GF = np.zeros((self.N, self.dv), np.int32)
        self.cn_weight = np.zeros(self.M, np.int32)
        self.cn_linkVNs = np.zeros((self.M, self.dc), np.int32)
        self.cn_linkVNs_GF = np.zeros((self.M, self.dc), np.int32)
        _check(lib.nbldpc_read_matrix(str(matrix_path).encode(), _np(dims), _np(self.vn_weight), _np(self.vn_linkCNs),
                                      _np(self.vn_linkCNs_GF), _np(self.cn_weight), _np(self.cn_linkVNs), _np(self.cn_linkVNs_GF)),
               "Get_H")
        self.rate = np.float32(self.N - self.M) / np.float32(self.N)  # H->rate (Simulation.cpp:365)


class NBCode(NBMatrix):
    """Get_H (Simulation.cpp:347-467) + device upload. Holds the flattened VN/CN arrays on the host too."""

    def __init__(self, matrix_path, TableMultiply):
        super().__init__(matrix_path)
        self.TableMultiply = np.ascontiguousarray(TableMultiply, np.uint32)
        h = c_void_p()
        _check(lib.nbldpc_code_create(self.N, self.M, self.q, self.dv, self.dc, _np(self.vn_weight), _np(self.vn_linkCNs),
                                      _np(self.vn_linkCNs_GF), _np(self.cn_weight), _np(self.cn_linkVNs), _np(self.cn_linkVNs_GF),
                                      _np(self.TableMultiply), ctypes.byref(h)), "nbldpc_code_create")
        self._h = h

    def _encoder_info(self):
        if getattr(self, "_info_pos", None) is None:
            k, r = c_int(0), c_int(0)
            pos = np.zeros(self.N, np.int32)
            _check(lib.nbldpc_encoder_info(self._h, ctypes.byref(k), ctypes.byref(r), _np(pos)), "nbldpc_encoder_info")
            self._K_info, self._rank, self._info_pos = k.value, r.value, pos[:k.value].copy()
        return self._K_info, self._rank, self._info_pos

    @property
    def K_info(self):
        """K' = N - rank(H): information symbols per codeword of the systematic encoder (builds the generator on first use)."""
        return self._encoder_info()[0]

    @property
    def rank(self):
        return self._encoder_info()[1]

    @property
    def info_positions(self):
        """int32 [K'] (host, ascending): codeword position of each information symbol."""
        return self._encoder_info()[2]

    @property
    def last_kernel(self):
        """Name of the kernel the last decode call on this code launched (nbldpc_last_kernel)."""
        return lib.nbldpc_last_kernel(self._h).decode()

    def grids(self):
        """nbldpc_code_grids: dict(persist_grid, pipe_grid, tmm_grid, tmm_grid_layered) -- a batch larger than a kernel's grid is
        decoded by its persistent form (frames from a counter)."""
        d = np.zeros(4, np.int32)
        _check(lib.nbldpc_code_grids(self._h, _np(d)), "nbldpc_code_grids")
        return dict(persist_grid=int(d[0]), pipe_grid=int(d[1]), tmm_grid=int(d[2]), tmm_grid_layered=int(d[3]))

    @property
    def qspa_layered_threads(self):
        """Threads per workgroup of k_nb_qspa_layered for this code (nbldpc_qspa_layered_threads): 256, 512 or 1024."""
        return int(lib.nbldpc_qspa_layered_threads(self._h))

    def qspa_ws_info(self, layered=False):
        """nbldpc_qspa_ws_info: the workspace tier's plan for this code, dict(threads, lds_bytes, slot_bytes, vectors), with the
        switches the code was created under (NBLDPC_QSPA_WS_THREADS).  Raises LdpcError where the plan refuses the code."""
        d = np.zeros(4, np.int32)
        _check(lib.nbldpc_qspa_ws_info(self._h, 1 if layered else 0, _np(d)), "nbldpc_qspa_ws_info")
        return dict(threads=int(d[0]), lds_bytes=int(d[1]), slot_bytes=int(d[2]), vectors=int(d[3]))

    def qspa_ws_slots(self, B, layered=False):
        """nbldpc_qspa_ws_slots: the workspace slots (= persistent workgroups) a workspace-tier call with B frames allocates on this
        code: min(B, 1024, what fits in 2 GiB, NBLDPC_QSPA_WS_SLOTS as read when the code was created)."""
        n = int(lib.nbldpc_qspa_ws_slots(self._h, 1 if layered else 0, B))
        _check(min(n, 0), "nbldpc_qspa_ws_slots")
        return n

    @property
    def persist_grid(self):
        return self.grids()["persist_grid"]

    def close(self):
        if getattr(self, "_h", None):
            lib.nbldpc_code_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def Decoding_EMS(code, L_ch, EMS_Nm=2, EMS_Nc=2, maxIT=20, maxdc=0, want_state=False, stream=None):
    """Decoding_EMS (LDPC_Decoder.cpp:172-317) for a batch.

    L_ch: CUDA float32 [B, N, q-1].  Returns dict(DecodeOutput [B,N] int32, iter_number [B], ok [B],
    LLR [B,N,q-1] | None, L_c2v [B,M,dc,q-1] | None), all on the device.  want_state: True = both state arrays,
    "llr" = VN[].LLR only (the two-frame pipeline kernel does not produce CN[].L_c2v: a call that asks for it runs on k_nb_ems)."""
    if not (L_ch.is_cuda and L_ch.dtype == torch.float32 and L_ch.is_contiguous()):
        raise ValueError("L_ch must be a contiguous CUDA float32 tensor")
    if L_ch.dim() != 3 or L_ch.shape[1] != code.N or L_ch.shape[2] != code.q - 1:
        raise ValueError("L_ch must be [B, N=%d, q-1=%d]" % (code.N, code.q - 1))
    B, dev = int(L_ch.shape[0]), L_ch.device
    out = torch.empty((B, code.N), dtype=torch.int32, device=dev)
    iters = torch.empty(B, dtype=torch.int32, device=dev)
    ok = torch.empty(B, dtype=torch.int32, device=dev)
    LLR = torch.empty((B, code.N, code.q - 1), dtype=torch.float32, device=dev) if want_state else None
    c2v = torch.empty((B, code.M, code.dc, code.q - 1), dtype=torch.float32, device=dev) if (want_state and want_state != "llr") else None
    st = c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)
    _check(lib.nbldpc_ems_decode_batch(code._h, _dev(L_ch), B, EMS_Nm, EMS_Nc, maxIT, maxdc, _dev(out), _dev(iters), _dev(ok),
                                       _dev(LLR), _dev(c2v), st), "Decoding_EMS")
    return dict(DecodeOutput=out, iter_number=iters, ok=ok, LLR=LLR, L_c2v=c2v)


def Decoding_TMM(code, L_ch, maxIT=20, layered=False, want_state=False, stream=None):
    """Decoding_TMM (LDPC_Decoder.cpp:361-558) / Decoding_layered_TMM (:560-702, layered=True) for a batch.
    Returns the same dict as Decoding_EMS; LLR [B,N,q] and L_c2v [B,M,dc,q] carry all q entries per vector."""
    if not (L_ch.is_cuda and L_ch.dtype == torch.float32 and L_ch.is_contiguous()):
        raise ValueError("L_ch must be a contiguous CUDA float32 tensor")
    if L_ch.dim() != 3 or L_ch.shape[1] != code.N or L_ch.shape[2] != code.q - 1:
        raise ValueError("L_ch must be [B, N=%d, q-1=%d]" % (code.N, code.q - 1))
    B, dev = int(L_ch.shape[0]), L_ch.device
    out = torch.empty((B, code.N), dtype=torch.int32, device=dev)
    iters = torch.empty(B, dtype=torch.int32, device=dev)
    ok = torch.empty(B, dtype=torch.int32, device=dev)
    LLR = torch.empty((B, code.N, code.q), dtype=torch.float32, device=dev) if want_state else None
    c2v = torch.empty((B, code.M, code.dc, code.q), dtype=torch.float32, device=dev) if want_state else None
    st = c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)
    _check(lib.nbldpc_tmm_decode_batch(code._h, _dev(L_ch), B, 1 if layered else 0, maxIT, _dev(out), _dev(iters), _dev(ok), _dev(LLR),
                                       _dev(c2v), st), "Decoding_TMM")
    return dict(DecodeOutput=out, iter_number=iters, ok=ok, LLR=LLR, L_c2v=c2v)


QSPA_LDS_LIMIT = 159 * 1024
QSPA_TIERS = ("lds", "workspace", "auto")


def qspa_lds_bytes(N, M, q, dc):
    """The frame state of the LDS tier of Decoding_QSPA (include/nbldpc.h, "FHT sum-product": the bound is QSPA_LDS_LIMIT)."""
    return 4 * (N * q + M * dc * q) + 4 * (N + 4) + q * q


def QSPA_WS_Plan_host(N, M, q, dc, widest_level=0, layered=False):
    """nbldpc_qspa_ws_plan_host: the plan of the workspace tier without a device, dict(threads, lds_bytes, slot_bytes, vectors).
    widest_level (the most rows any dependency level holds) is read for layered=True only.  Raises LdpcError on a refusal."""
    d = np.zeros(4, np.int32)
    _check(lib.nbldpc_qspa_ws_plan_host(N, M, q, dc, widest_level, 1 if layered else 0, _np(d)), "QSPA_WS_Plan_host")
    return dict(threads=int(d[0]), lds_bytes=int(d[1]), slot_bytes=int(d[2]), vectors=int(d[3]))


def Decoding_QSPA(code, L_ch, maxIT=20, want_state=False, stream=None, layered=False, tier="lds"):
    """nbldpc_qspa_decode_batch: the FHT sum-product decoder (include/nbldpc.h, "FHT sum-product"; ours, the reference has none) for
    a batch; layered=True: nbldpc_qspa_layered_decode_batch, the row-by-row schedule ("FHT sum-product, layered schedule").  Returns
    the dict of Decoding_TMM: LLR [B,N,q] holds the APP probability vectors of the last executed iteration, L_c2v [B,M,dc,q] the
    check-to-variable vectors, all q entries each, max-normalised with the floor 2^-40.
    tier: "lds" the calls above (a code whose frame state exceeds QSPA_LDS_LIMIT is refused); "workspace"
    nbldpc_qspa_ws_decode_batch, the frame's vectors in a global-memory workspace ("FHT sum-product, workspace tier"); "auto" the LDS
    call where qspa_lds_bytes fits, else the workspace call.  The results do not depend on it."""
    if tier not in QSPA_TIERS:
        raise ValueError("tier must be one of %s, not %r" % (", ".join(QSPA_TIERS), tier))
    if not (L_ch.is_cuda and L_ch.dtype == torch.float32 and L_ch.is_contiguous()):
        raise ValueError("L_ch must be a contiguous CUDA float32 tensor")
    if L_ch.dim() != 3 or L_ch.shape[1] != code.N or L_ch.shape[2] != code.q - 1:
        raise ValueError("L_ch must be [B, N=%d, q-1=%d]" % (code.N, code.q - 1))
    B, dev = int(L_ch.shape[0]), L_ch.device
    out = torch.empty((B, code.N), dtype=torch.int32, device=dev)
    iters = torch.empty(B, dtype=torch.int32, device=dev)
    ok = torch.empty(B, dtype=torch.int32, device=dev)
    APP = torch.empty((B, code.N, code.q), dtype=torch.float32, device=dev) if want_state else None
    c2v = torch.empty((B, code.M, code.dc, code.q), dtype=torch.float32, device=dev) if want_state else None
    st = c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)
    if tier == "workspace" or (tier == "auto" and qspa_lds_bytes(code.N, code.M, code.q, code.dc) > QSPA_LDS_LIMIT):
        _check(lib.nbldpc_qspa_ws_decode_batch(code._h, _dev(L_ch), B, 1 if layered else 0, maxIT, _dev(out), _dev(iters), _dev(ok), _dev(APP),
                                               _dev(c2v), st), "Decoding_QSPA")
        return dict(DecodeOutput=out, iter_number=iters, ok=ok, LLR=APP, L_c2v=c2v)
    call = lib.nbldpc_qspa_layered_decode_batch if layered else lib.nbldpc_qspa_decode_batch
    _check(call(code._h, _dev(L_ch), B, maxIT, _dev(out), _dev(iters), _dev(ok), _dev(APP), _dev(c2v), st), "Decoding_QSPA")
    return dict(DecodeOutput=out, iter_number=iters, ok=ok, LLR=APP, L_c2v=c2v)


def Decoding_QSPA_host(code, L_ch, maxIT=20, want_state=False, TableMultiply=None, layered=False):
    """nbldpc_qspa_decode_host (layered=True: nbldpc_qspa_layered_decode_host): the host statement of Decoding_QSPA on host arrays, no
    device needed.  code: an NBMatrix or NBCode (TableMultiply: the code's unless given); L_ch float32 [B, N, q-1].  Returns the same
    dict, numpy arrays."""
    mul = np.ascontiguousarray(code.TableMultiply if TableMultiply is None else TableMultiply, np.uint32)
    if mul.shape != (code.q, code.q):
        raise ValueError("TableMultiply must be [q, q]")
    L = np.ascontiguousarray(L_ch, np.float32)
    if L.ndim != 3 or L.shape[0] <= 0 or L.shape[1:] != (code.N, code.q - 1):
        raise ValueError("L_ch must be float32 [B, N=%d, q-1=%d]" % (code.N, code.q - 1))
    B = L.shape[0]
    out, iters, ok = np.empty((B, code.N), np.int32), np.empty(B, np.int32), np.empty(B, np.int32)
    APP = np.empty((B, code.N, code.q), np.float32) if want_state else None
    c2v = np.empty((B, code.M, code.dc, code.q), np.float32) if want_state else None
    call = lib.nbldpc_qspa_layered_decode_host if layered else lib.nbldpc_qspa_decode_host
    _check(call(code.N, code.M, code.q, code.dv, code.dc, _np(code.vn_weight), _np(code.vn_linkCNs), _np(code.vn_linkCNs_GF),
                                       _np(code.cn_weight), _np(code.cn_linkVNs), _np(code.cn_linkVNs_GF), _np(mul), _np(L), B, maxIT, _np(out),
                                       _np(iters), _np(ok), None if APP is None else _np(APP), None if c2v is None else _np(c2v)),
           "Decoding_QSPA_host")
    return dict(DecodeOutput=out, iter_number=iters, ok=ok, LLR=APP, L_c2v=c2v)


def QSPA_Exp_host(x):
    """nbldpc_qspa_exp_host: the decoder's shared exponential (x <= 0) on a host array, elementwise."""
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    _check(lib.nbldpc_qspa_exp_host(_np(x), x.size, _np(y)), "QSPA_Exp_host")
    return y


def Get_CONSTELLATION(path, n_QAM):
    """Get_CONSTELLATION (Simulation.cpp:313-338) -> host float32 [n_QAM, 2] (Real, Image)."""
    con = np.zeros((n_QAM, 2), np.float32)
    _check(lib.nbldpc_read_constellation(str(path).encode(), n_QAM, _np(con)), "Get_CONSTELLATION")
    return con


def Demodulate(code, rx, sigma, stream=None, CONSTELLATION=None):
    """Demodulate on the device.  BPSK branch (LDPC_Decoder.cpp:132-157): rx [B, N*m] -> L_ch [B, N, q-1].  With
    CONSTELLATION (CUDA float32 [q, 2]) the n_QAM != 2 branch (:160-169): rx [B, N, 2] (include/nbldpc.h)."""
    if CONSTELLATION is not None:
        if not (rx.is_cuda and rx.dtype == torch.float32 and rx.is_contiguous() and rx.dim() == 3 and tuple(rx.shape[1:]) == (code.N, 2)):
            raise ValueError("rx must be a contiguous CUDA float32 tensor [B, N, 2]")
        if not (CONSTELLATION.is_cuda and CONSTELLATION.dtype == torch.float32 and CONSTELLATION.is_contiguous()
                and tuple(CONSTELLATION.shape) == (code.q, 2)):
            raise ValueError("CONSTELLATION must be a contiguous CUDA float32 tensor [q, 2]")
        B = int(rx.shape[0])
        Lch = torch.empty((B, code.N, code.q - 1), dtype=torch.float32, device=rx.device)
        st = c_void_p((stream or torch.cuda.current_stream(rx.device)).cuda_stream)
        _check(lib.nbldpc_demodulate_qam(code._h, _dev(rx), _dev(CONSTELLATION), c_float(sigma), B, _dev(Lch), st), "Demodulate")
        return Lch
    if not (rx.is_cuda and rx.dtype == torch.float32 and rx.is_contiguous() and rx.dim() == 2 and rx.shape[1] == code.N * code.m):
        raise ValueError("rx must be a contiguous CUDA float32 tensor [B, N*m]")
    B = int(rx.shape[0])
    Lch = torch.empty((B, code.N, code.q - 1), dtype=torch.float32, device=rx.device)
    st = c_void_p((stream or torch.cuda.current_stream(rx.device)).cuda_stream)
    _check(lib.nbldpc_demodulate_bpsk(code._h, _dev(rx), c_float(sigma), B, _dev(Lch), st), "Demodulate")
    return Lch


def _check_qam_fading(code, rx, gain, CONSTELLATION):
    if not (torch.is_tensor(rx) and rx.is_cuda and rx.dtype == torch.float32 and rx.is_contiguous() and rx.dim() == 3
            and tuple(rx.shape[1:]) == (code.N, 2) and rx.shape[0] > 0):
        raise ValueError("rx must be a contiguous CUDA float32 tensor [B, N, 2]")
    if not (torch.is_tensor(CONSTELLATION) and CONSTELLATION.is_cuda and CONSTELLATION.dtype == torch.float32 and CONSTELLATION.is_contiguous()
            and tuple(CONSTELLATION.shape) == (code.q, 2)):
        raise ValueError("CONSTELLATION must be a contiguous CUDA float32 tensor [q, 2]")
    if not (torch.is_tensor(gain) and gain.is_cuda and gain.device == rx.device and gain.dtype == torch.float32 and gain.is_contiguous()
            and tuple(gain.shape) == (int(rx.shape[0]), code.N)):
        raise ValueError("gain must be a contiguous CUDA float32 tensor [B=%d, N=%d] on %s" % (rx.shape[0], code.N, rx.device))


def Demodulate_QAM_Fading(code, rx, gain, sigma, CONSTELLATION, stream=None):
    """nbldpc_demodulate_qam_fading: the n_QAM != 2 branch of Demodulate against the faded points gain[b, s] * c_k (receiver CSI).
    rx CUDA float32 [B, N, 2], gain CUDA float32 [B, N], CONSTELLATION CUDA float32 [q, 2] -> L_ch [B, N, q-1]; a gain of 1 gives
    Demodulate's bits."""
    _check_qam_fading(code, rx, gain, CONSTELLATION)
    B = int(rx.shape[0])
    Lch = torch.empty((B, code.N, code.q - 1), dtype=torch.float32, device=rx.device)
    st = c_void_p((stream or torch.cuda.current_stream(rx.device)).cuda_stream)
    _check(lib.nbldpc_demodulate_qam_fading(code._h, _dev(rx), _dev(gain), _dev(CONSTELLATION), c_float(sigma), B, _dev(Lch), st),
           "Demodulate_QAM_Fading")
    return Lch


def Demodulate_QAM_Fading_host(N, q, rx, gain, CONSTELLATION, sigma):
    """nbldpc_demodulate_qam_fading_host: the statement of Demodulate_QAM_Fading on host arrays.  rx [B, N, 2], gain [B, N] -> [B, N, q-1]."""
    rx = np.ascontiguousarray(rx, np.float32)
    con = np.ascontiguousarray(CONSTELLATION, np.float32)
    if rx.ndim != 3 or rx.shape[0] <= 0 or tuple(rx.shape[1:]) != (N, 2) or con.shape != (q, 2):
        raise ValueError("rx must be float32 [B, N=%d, 2] and CONSTELLATION float32 [q=%d, 2]" % (N, q))
    g = np.ascontiguousarray(gain, np.float32)
    if g.shape != rx.shape[:2]:
        raise ValueError("gain must be float32 [B, N]")
    Lch = np.empty((rx.shape[0], N, q - 1), np.float32)
    _check(lib.nbldpc_demodulate_qam_fading_host(N, q, _np(rx), _np(g), _np(con), c_float(sigma), rx.shape[0], _np(Lch)), "Demodulate_QAM_Fading_host")
    return Lch


def AWGNChannel_Fading_GPU(seed, sigma, code, CodeWord_sym_dev, gain, CONSTELLATION, stream=None):
    """nbldpc_fading_channel_device_qam_frames for a GF(q) code over q-QAM: frame b sends row b of CodeWord_sym_dev (CUDA int32 [B, N]),
    the point of symbol (b, i) scaled by gain[b, i] (CUDA float32 [B, N]) before the noise of AWGNChannel_GPU's per-frame QAM form is
    added: the same four draws per symbol, the same seed advance.  Returns rx CUDA float32 [B, N, 2]."""
    if not (isinstance(seed, np.ndarray) and seed.dtype == np.int32 and seed.size == 3):
        raise ValueError("seed must be an int32 numpy array of 3")
    if not (torch.is_tensor(CodeWord_sym_dev) and CodeWord_sym_dev.is_cuda and CodeWord_sym_dev.dtype == torch.int32 and CodeWord_sym_dev.is_contiguous()
            and CodeWord_sym_dev.dim() == 2 and CodeWord_sym_dev.shape[1] == code.N and CodeWord_sym_dev.shape[0] > 0):
        raise ValueError("CodeWord_sym_dev must be a contiguous CUDA int32 tensor [B, N=%d]" % code.N)
    B = int(CodeWord_sym_dev.shape[0])
    rx = torch.empty((B, code.N, 2), dtype=torch.float32, device=CodeWord_sym_dev.device)
    _check_qam_fading(code, rx, gain, CONSTELLATION)
    st = c_void_p((stream or torch.cuda.current_stream(rx.device)).cuda_stream)
    _check(lib.nbldpc_fading_channel_device_qam_frames(_np(seed), c_float(sigma), _dev(CodeWord_sym_dev), code.N, _dev(CONSTELLATION), code.q,
                                                       _dev(gain), B, _dev(rx), st), "AWGNChannel_Fading_GPU")
    return rx


def AWGNChannel_CPU(seed, sigma, code, CodeWord_sym, CONSTELLATION=None):
    """Modulate + AWGNChannel_CPU (LDPC_Encoder.cpp:18-68) for ONE frame; seed advanced.  BPSK -> host rx [N*m]; with
    CONSTELLATION (host float32 [q, 2]) the n_QAM != 2 branch -> host rx [N, 2]."""
    if not (isinstance(seed, np.ndarray) and seed.dtype == np.int32 and seed.size == 3):
        raise ValueError("seed must be an int32 numpy array of 3")
    cw = np.ascontiguousarray(CodeWord_sym, np.int32)
    if CONSTELLATION is not None:
        con = np.ascontiguousarray(CONSTELLATION, np.float32)
        rx = np.empty((code.N, 2), np.float32)
        _check(lib.nbldpc_awgn_channel_host_qam(_np(seed), c_float(sigma), _np(cw), code.N, _np(con), con.shape[0], _np(rx)), "AWGNChannel_CPU")
        return rx
    rx = np.empty(code.N * code.m, np.float32)
    _check(lib.nbldpc_awgn_channel_host(_np(seed), c_float(sigma), _np(cw), code.N, code.m, _np(rx)), "AWGNChannel_CPU")
    return rx


def AWGNChannel_GPU(seed, sigma, code, CodeWord_sym_dev, B, stream=None, CONSTELLATION=None):
    """Device-side Modulate + AWGNChannel for B consecutive frames of the same stream (LCG jump-ahead: the uniforms are
    the reference's, the samples may differ from the host libm's by an ulp).  Returns rx CUDA float32 [B, N*m]; seed
    advanced exactly like B calls of AWGNChannel_CPU.  CodeWord_sym_dev [N] is sent by every frame; [B, N] (contiguous) gives
    frame b its own word, row b, with the same draws."""
    if not (isinstance(seed, np.ndarray) and seed.dtype == np.int32 and seed.size == 3):
        raise ValueError("seed must be an int32 numpy array of 3")
    per_frame = CodeWord_sym_dev.dim() == 2
    if per_frame:
        if not (CodeWord_sym_dev.is_cuda and CodeWord_sym_dev.dtype == torch.int32 and CodeWord_sym_dev.is_contiguous()
                and tuple(CodeWord_sym_dev.shape) == (B, code.N)):
            raise ValueError("CodeWord_sym_dev must be a contiguous CUDA int32 tensor [B=%d, N=%d]" % (B, code.N))
    elif not (CodeWord_sym_dev.is_cuda and CodeWord_sym_dev.dtype == torch.int32 and CodeWord_sym_dev.numel() == code.N):
        raise ValueError("CodeWord_sym_dev must be a CUDA int32 tensor of N symbols")
    if CONSTELLATION is not None:  # n_QAM != 2 branch: rx [B, N, 2], four draws per SYMBOL
        if not (CONSTELLATION.is_cuda and CONSTELLATION.dtype == torch.float32 and CONSTELLATION.is_contiguous()
                and tuple(CONSTELLATION.shape) == (code.q, 2)):
            raise ValueError("CONSTELLATION must be a contiguous CUDA float32 tensor [q, 2]")
        rx = torch.empty((B, code.N, 2), dtype=torch.float32, device=CodeWord_sym_dev.device)
        st = c_void_p((stream or torch.cuda.current_stream(rx.device)).cuda_stream)
        if per_frame:
            _check(lib.nbldpc_awgn_channel_device_qam_frames(_np(seed), c_float(sigma), _dev(CodeWord_sym_dev), code.N, _dev(CONSTELLATION), code.q,
                                                             B, _dev(rx), st), "AWGNChannel_GPU")
        else:
            _check(lib.nbldpc_awgn_channel_device_qam(_np(seed), c_float(sigma), _dev(CodeWord_sym_dev), code.N, _dev(CONSTELLATION), B, _dev(rx), st),
                   "AWGNChannel_GPU")
        return rx
    rx = torch.empty((B, code.N * code.m), dtype=torch.float32, device=CodeWord_sym_dev.device)
    st = c_void_p((stream or torch.cuda.current_stream(rx.device)).cuda_stream)
    fn = lib.nbldpc_awgn_channel_device_frames if per_frame else lib.nbldpc_awgn_channel_device
    _check(fn(_np(seed), c_float(sigma), _dev(CodeWord_sym_dev), code.N, code.m, B, _dev(rx), st), "AWGNChannel_GPU")
    return rx


def seed_after(seed, frames, code, qam=False, E=None):
    """The RandomModule state after `frames` more frames (4 draws per bit; per symbol with a QAM constellation).  E: the transmitted
    symbols per frame of a rate-matched transmission, in place of code.N."""
    a, m = (249, 251, 252), (61967, 63443, 63599)
    k = 4 * (code.N if E is None else int(E)) * (1 if qam else code.m) * int(frames)
    return np.array([(int(seed[i]) * pow(a[i], k, m[i])) % m[i] for i in range(3)], np.int32)


def sigma_of(SNR, rate, snrtype=0, n_QAM=2):
    """sigma of a sweep point (main.cu:221-228); snrtype 0 = Eb/N0 (reference default, define.h:45)."""
    return float(lib.nbldpc_sigma(np.float32(SNR), snrtype, n_QAM, np.float32(rate)))


def Statistic(code, counters, res, CodeWord_sym_dev, stream=None):
    """Statistic (Simulation.cpp:256-279) on the device; counters: CUDA int64[4], accumulated.  CodeWord_sym_dev [N] for every
    frame, or [B, N] (contiguous): frame b against row b."""
    B = int(res["DecodeOutput"].shape[0])
    st = c_void_p((stream or torch.cuda.current_stream(counters.device)).cuda_stream)
    if CodeWord_sym_dev.dim() == 2:
        if not (CodeWord_sym_dev.is_contiguous() and CodeWord_sym_dev.dtype == torch.int32 and tuple(CodeWord_sym_dev.shape) == (B, code.N)):
            raise ValueError("CodeWord_sym_dev must be a contiguous int32 tensor [B=%d, N=%d]" % (B, code.N))
        fn = lib.nbldpc_statistic_frames
    else:
        fn = lib.nbldpc_statistic
    _check(fn(code._h, _dev(res["DecodeOutput"]), _dev(res["iter_number"]), _dev(res["ok"]), _dev(CodeWord_sym_dev), B, _dev(counters), st),
           "Statistic")


def generator_host(code, TableMultiply=None):
    """nbldpc_generator_host: the systematic generator on the host (no device), from the CN lists of an NBMatrix / NBCode and
    TableMultiply (default: the code's).  Returns dict(K_info, rank, info_pos=int32 [K'], P=uint8 [rank, K']): parity symbol r
    (the r-th non-information position, ascending) = XOR_j TableMultiply[msg[j]][P[r, j]]."""
    mul = np.ascontiguousarray(code.TableMultiply if TableMultiply is None else TableMultiply, np.uint32)
    if mul.shape != (code.q, code.q):
        raise ValueError("TableMultiply must be [q, q]")
    k, r = c_int(0), c_int(0)
    pos = np.zeros(code.N, np.int32)
    P = np.zeros(code.N * code.N // 4 + 1, np.uint8)  # rank * K' <= N^2 / 4: one call fills both
    _check(lib.nbldpc_generator_host(code.N, code.M, code.q, code.dc, _np(code.cn_weight), _np(code.cn_linkVNs), _np(code.cn_linkVNs_GF), _np(mul),
                                     ctypes.byref(k), ctypes.byref(r), _np(pos), _np(P)), "nbldpc_generator_host")
    return dict(K_info=k.value, rank=r.value, info_pos=pos[:k.value].copy(), P=P[:r.value * k.value].reshape(r.value, k.value).copy())


def _check_cw(CodeWord_sym, B, N, dev):
    if not (torch.is_tensor(CodeWord_sym) and CodeWord_sym.is_cuda and CodeWord_sym.device == dev and CodeWord_sym.dtype == torch.int32
            and CodeWord_sym.is_contiguous() and tuple(CodeWord_sym.shape) == (B, N)):
        raise ValueError("CodeWord_sym must be a contiguous CUDA int32 tensor [B=%d, N=%d] on %s" % (B, N, dev))


def Encode(code, msg, CodeWord_sym=None, stream=None):
    """nbldpc_encode: msg = CUDA int32 tensor [B, K'] (low log2 q bits read) -> CodeWord_sym int32 [B, N] on the device,
    systematic on code.info_positions."""
    K = code.K_info
    if not (torch.is_tensor(msg) and msg.is_cuda and msg.dtype == torch.int32 and msg.is_contiguous() and msg.dim() == 2
            and msg.shape[1] == K and msg.shape[0] > 0):
        raise ValueError("msg must be a contiguous CUDA int32 tensor [B, K'=%d]" % K)
    B, dev = int(msg.shape[0]), msg.device
    if CodeWord_sym is None:
        CodeWord_sym = torch.empty((B, code.N), dtype=torch.int32, device=dev)
    else:
        _check_cw(CodeWord_sym, B, code.N, dev)
    st = c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)
    _check(lib.nbldpc_encode(code._h, _dev(msg), B, _dev(CodeWord_sym), st), "Encode")
    return CodeWord_sym


def PN_CodeWords(code, seed, B, first_frame=0, want_msg=False, device=None, CodeWord_sym=None, stream=None, rate_match=None):
    """nbldpc_encode_random: the codewords of frames first_frame .. first_frame+B-1 of the message stream `seed` (counter-based
    rule of nbldpc.h, mirrored by pn_messages below).  Returns CodeWord_sym int32 [B, N] on the device, or (CodeWord_sym,
    msg [B, K']) with want_msg.  rate_match (a RateMatch over code.N symbols): nbldpc_rm_encode_random -- the message symbols at the
    profile's shortened positions are forced to 0 before encoding (msg: after the forcing); the shortened positions must lie in the
    information set."""
    if B <= 0 or first_frame < 0:
        raise ValueError("B must be positive and first_frame >= 0")
    device = device or torch.device("cuda", torch.cuda.current_device())
    if CodeWord_sym is None:
        CodeWord_sym = torch.empty((B, code.N), dtype=torch.int32, device=device)
    else:
        _check_cw(CodeWord_sym, B, code.N, device)
    msg = torch.empty((B, code.K_info), dtype=torch.int32, device=device) if (want_msg or rate_match is not None) else None
    st = c_void_p((stream or torch.cuda.current_stream(device)).cuda_stream)
    if rate_match is not None:
        _check(lib.nbldpc_rm_encode_random(code._h, rate_match._h, ctypes.c_ulonglong(int(seed) % (1 << 64)), int(first_frame), B, _dev(msg),
                                           _dev(CodeWord_sym), st), "PN_CodeWords")
        return (CodeWord_sym, msg) if want_msg else CodeWord_sym
    _check(lib.nbldpc_encode_random(code._h, ctypes.c_ulonglong(int(seed) % (1 << 64)), int(first_frame), B, _dev(msg), _dev(CodeWord_sym), st),
           "PN_CodeWords")
    return (CodeWord_sym, msg) if want_msg else CodeWord_sym


def pn_messages(seed, K_info, q, B, first_frame=0):
    """Host mirror of nbldpc_encode_random's message rule: int32 [B, K']."""
    from .bldpc import splitmix64
    m = int(q).bit_length() - 1
    s = 64 // m
    W = -(-K_info // s)
    g = np.arange(first_frame, first_frame + B, dtype=np.uint64)
    k = np.arange(K_info)
    with np.errstate(over="ignore"):
        ctr = np.uint64(int(seed) % (1 << 64)) + g[:, None] * np.uint64(W) + (k // s).astype(np.uint64)[None, :]
    words = splitmix64(ctr)
    return ((words >> (m * (k % s)).astype(np.uint64)[None, :]) & np.uint64(q - 1)).astype(np.int32)


def Syndrome(code, DecodeOutput, stream=None):
    """nbldpc_syndrome: H * d_b == 0 over GF(q) for every frame of DecodeOutput (CUDA int32 [B, N], low log2 q bits read).
    Returns dict(flag=int32 [B], unsat=int32 [B]: unsatisfied checks) on the device."""
    if not (torch.is_tensor(DecodeOutput) and DecodeOutput.is_cuda and DecodeOutput.dtype == torch.int32 and DecodeOutput.is_contiguous()
            and DecodeOutput.dim() == 2 and DecodeOutput.shape[1] == code.N and DecodeOutput.shape[0] > 0):
        raise ValueError("DecodeOutput must be a contiguous CUDA int32 tensor [B, N=%d]" % code.N)
    B, dev = int(DecodeOutput.shape[0]), DecodeOutput.device
    flag = torch.empty(B, dtype=torch.int32, device=dev)
    unsat = torch.empty(B, dtype=torch.int32, device=dev)
    st = c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)
    _check(lib.nbldpc_syndrome(code._h, _dev(DecodeOutput), B, _dev(flag), _dev(unsat), st), "Syndrome")
    return dict(flag=flag, unsat=unsat)


# ---- rate matching over symbol LLR vectors (include/nbldpc.h, "rate matching").  A profile is a bldpc.RateMatch made with N = code.N
# symbols; q is the field size (an int, or anything with a .q: a code); every array is frame-outer. ----
def _q_of(q):
    q = int(getattr(q, "q", q))
    if q < 2 or q > 256 or q & (q - 1):
        raise ValueError("q=%d is not a power of two in 2 .. 256" % q)
    return q, q.bit_length() - 1


def _check_short_llr(short_llr):
    if not (np.isfinite(short_llr) and short_llr > 0):
        raise ValueError("short_llr must be finite and > 0, not %r" % (short_llr,))


def _rm_dev(t, shape_tail, dtype, what, B=None, dev=None):
    """t: a contiguous CUDA tensor [B, *shape_tail] of dtype (on dev, with B frames, when given).  Returns (B, device)."""
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.dim() == 1 + len(shape_tail)
            and tuple(t.shape[1:]) == tuple(shape_tail) and t.shape[0] > 0 and (B is None or t.shape[0] == B) and (dev is None or t.device == dev)):
        raise ValueError("%s must be a contiguous CUDA %s tensor [B%s, %s]%s" % (what, str(dtype).split(".")[-1], "" if B is None else "=%d" % B,
                                                                               ", ".join(str(s) for s in shape_tail), "" if dev is None else " on %s" % dev))
    return int(t.shape[0]), t.device


def _rm_host(a, shape_tail, dtype, what, B=None):
    a = np.ascontiguousarray(a, dtype)
    if a.ndim != 1 + len(shape_tail) or tuple(a.shape[1:]) != tuple(shape_tail) or a.shape[0] <= 0 or (B is not None and a.shape[0] != B):
        raise ValueError("%s must be %s [B%s, %s]" % (what, np.dtype(dtype).name, "" if B is None else "=%d" % B, ", ".join(str(s) for s in shape_tail)))
    return a


def _rm_done(done, B, dev):
    if done is not None and not (torch.is_tensor(done) and done.is_cuda and done.device == dev and done.dtype == torch.int32 and done.dim() == 1
                                 and done.is_contiguous() and done.shape[0] == B):
        raise ValueError("done must be a contiguous CUDA int32 tensor [B=%d] on %s (a decoder's ok will do)" % (B, dev))


def _rm_done_host(done, B):
    if done is None:
        return None
    done = np.ascontiguousarray(done, np.int32)
    if done.shape != (B,):
        raise ValueError("done must be int32 [B=%d]" % B)
    return done


def _rm_acc_host(acc, N, V):
    if not (isinstance(acc, np.ndarray) and acc.dtype == np.float32 and acc.flags.c_contiguous and acc.ndim == 3 and acc.shape[0] > 0
            and acc.shape[1:] == (N, V)):
        raise ValueError("L_acc must be a C-contiguous float32 array [B, N=%d, q-1=%d], updated in place" % (N, V))
    return acc


def _rm_con(CONSTELLATION, q, dev=None):
    if dev is None:
        con = np.ascontiguousarray(CONSTELLATION, np.float32)
        if con.shape != (q, 2):
            raise ValueError("CONSTELLATION must be float32 [q=%d, 2]" % q)
        return con
    if not (torch.is_tensor(CONSTELLATION) and CONSTELLATION.is_cuda and CONSTELLATION.device == dev and CONSTELLATION.dtype == torch.float32
            and CONSTELLATION.is_contiguous() and tuple(CONSTELLATION.shape) == (q, 2)):
        raise ValueError("CONSTELLATION must be a contiguous CUDA float32 tensor [q=%d, 2] on %s" % (q, dev))
    return CONSTELLATION


def _stream(stream, dev):
    return c_void_p((stream or torch.cuda.current_stream(dev)).cuda_stream)


def RM_Select(rm, CodeWord_sym, stream=None):
    """nbldpc_rm_select: CodeWord_sym CUDA int32 [B, N] -> the transmitted symbols int32 [B, E], tx[b, e] = CodeWord_sym[b, tx_pos[e]]."""
    B, dev = _rm_dev(CodeWord_sym, (rm.N,), torch.int32, "CodeWord_sym")
    tx = torch.empty((B, rm.E), dtype=torch.int32, device=dev)
    _check(lib.nbldpc_rm_select(rm._h, _dev(CodeWord_sym), B, _dev(tx), _stream(stream, dev)), "RM_Select")
    return tx


def RM_Select_host(rm, CodeWord_sym):
    """nbldpc_rm_select_host: RM_Select on a host array int32 [B, N], no device needed."""
    cw = _rm_host(CodeWord_sym, (rm.N,), np.int32, "CodeWord_sym")
    tx = np.empty((cw.shape[0], rm.E), np.int32)
    _check(lib.nbldpc_rm_select_host(rm._h, _np(cw), cw.shape[0], _np(tx)), "RM_Select_host")
    return tx


def RM_Recover(rm, q, Lrx, short_llr=1.0e4, stream=None):
    """nbldpc_rm_recover: received vectors Lrx CUDA float32 [B, E, q-1] -> L_ch [B, N, q-1]: a position's contributions added in
    ascending e (one contribution: the same bits), +0.0 on punctured and unreached positions, -short_llr on shortened ones."""
    q, _ = _q_of(q)
    B, dev = _rm_dev(Lrx, (rm.E, q - 1), torch.float32, "Lrx")
    _check_short_llr(short_llr)
    Lch = torch.empty((B, rm.N, q - 1), dtype=torch.float32, device=dev)
    _check(lib.nbldpc_rm_recover(rm._h, q, _dev(Lrx), B, c_float(short_llr), _dev(Lch), _stream(stream, dev)), "RM_Recover")
    return Lch


def RM_Recover_host(rm, q, Lrx, short_llr=1.0e4):
    """nbldpc_rm_recover_host: RM_Recover on a host array float32 [B, E, q-1], no device needed."""
    q, _ = _q_of(q)
    Lrx = _rm_host(Lrx, (rm.E, q - 1), np.float32, "Lrx")
    Lch = np.empty((Lrx.shape[0], rm.N, q - 1), np.float32)
    _check(lib.nbldpc_rm_recover_host(rm._h, q, _np(Lrx), Lrx.shape[0], c_float(short_llr), _np(Lch)), "RM_Recover_host")
    return Lch


def RM_Combine(rm, q, Lrx, L_acc, done=None, short_llr=1.0e4, stream=None):
    """nbldpc_rm_combine: add one more transmission Lrx CUDA float32 [B, E, q-1] into L_acc [B, N, q-1] in place (and return it):
    ((acc + Lrx[e_0]) + Lrx[e_1]) + ...; shortened positions become -short_llr; positions without a contribution and the frames with
    done[b] != 0 (CUDA int32 [B], e.g. a decoder's ok) keep their bits."""
    q, _ = _q_of(q)
    B, dev = _rm_dev(L_acc, (rm.N, q - 1), torch.float32, "L_acc")
    _rm_dev(Lrx, (rm.E, q - 1), torch.float32, "Lrx", B, dev)
    _check_short_llr(short_llr)
    _rm_done(done, B, dev)
    _check(lib.nbldpc_rm_combine(rm._h, q, _dev(Lrx), B, c_float(short_llr), _dev(done), _dev(L_acc), _stream(stream, dev)), "RM_Combine")
    return L_acc


def RM_Combine_host(rm, q, Lrx, L_acc, done=None, short_llr=1.0e4):
    """nbldpc_rm_combine_host: RM_Combine on host arrays; L_acc float32 [B, N, q-1] (C-contiguous) is updated in place."""
    q, _ = _q_of(q)
    acc = _rm_acc_host(L_acc, rm.N, q - 1)
    B = acc.shape[0]
    Lrx = _rm_host(Lrx, (rm.E, q - 1), np.float32, "Lrx", B)
    done = _rm_done_host(done, B)
    _check(lib.nbldpc_rm_combine_host(rm._h, q, _np(Lrx), B, c_float(short_llr), None if done is None else _np(done), _np(acc)), "RM_Combine_host")
    return acc


def RM_Demodulate_Recover(rm, q, rx, sigma, short_llr=1.0e4, stream=None, CONSTELLATION=None):
    """The fused receive of a first transmission: Demodulate at N := E followed by RM_Recover, bit for bit, from one kernel and
    without the [B, E, q-1] array.  BPSK: rx CUDA float32 [B, E*m]; with CONSTELLATION (CUDA float32 [q, 2]): rx [B, E, 2]."""
    q, m = _q_of(q)
    _check_short_llr(short_llr)
    if CONSTELLATION is not None:
        B, dev = _rm_dev(rx, (rm.E, 2), torch.float32, "rx")
        con = _rm_con(CONSTELLATION, q, dev)
        Lch = torch.empty((B, rm.N, q - 1), dtype=torch.float32, device=dev)
        _check(lib.nbldpc_rm_demodulate_qam_recover(rm._h, q, _dev(rx), _dev(con), c_float(sigma), B, c_float(short_llr), _dev(Lch),
                                                    _stream(stream, dev)), "RM_Demodulate_Recover")
        return Lch
    B, dev = _rm_dev(rx, (rm.E * m,), torch.float32, "rx")
    Lch = torch.empty((B, rm.N, q - 1), dtype=torch.float32, device=dev)
    _check(lib.nbldpc_rm_demodulate_bpsk_recover(rm._h, q, _dev(rx), c_float(sigma), B, c_float(short_llr), _dev(Lch), _stream(stream, dev)),
           "RM_Demodulate_Recover")
    return Lch


def RM_Demodulate_Combine(rm, q, rx, sigma, L_acc, done=None, short_llr=1.0e4, stream=None, CONSTELLATION=None):
    """The fused receive of a retransmission: Demodulate at N := E followed by RM_Combine into L_acc [B, N, q-1] under done, bit for
    bit, from one kernel.  rx as RM_Demodulate_Recover."""
    q, m = _q_of(q)
    _check_short_llr(short_llr)
    B, dev = _rm_dev(L_acc, (rm.N, q - 1), torch.float32, "L_acc")
    _rm_done(done, B, dev)
    if CONSTELLATION is not None:
        _rm_dev(rx, (rm.E, 2), torch.float32, "rx", B, dev)
        con = _rm_con(CONSTELLATION, q, dev)
        _check(lib.nbldpc_rm_demodulate_qam_combine(rm._h, q, _dev(rx), _dev(con), c_float(sigma), B, c_float(short_llr), _dev(done), _dev(L_acc),
                                                    _stream(stream, dev)), "RM_Demodulate_Combine")
        return L_acc
    _rm_dev(rx, (rm.E * m,), torch.float32, "rx", B, dev)
    _check(lib.nbldpc_rm_demodulate_bpsk_combine(rm._h, q, _dev(rx), c_float(sigma), B, c_float(short_llr), _dev(done), _dev(L_acc),
                                                 _stream(stream, dev)), "RM_Demodulate_Combine")
    return L_acc


def RM_Demodulate_Recover_host(rm, q, rx, sigma, short_llr=1.0e4, CONSTELLATION=None):
    """The host statement of RM_Demodulate_Recover: Demodulate_host at N := E, then RM_Recover_host."""
    q, m = _q_of(q)
    if CONSTELLATION is not None:
        rx, con = _rm_host(rx, (rm.E, 2), np.float32, "rx"), _rm_con(CONSTELLATION, q)
        Lch = np.empty((rx.shape[0], rm.N, q - 1), np.float32)
        _check(lib.nbldpc_rm_demodulate_qam_recover_host(rm._h, q, _np(rx), _np(con), c_float(sigma), rx.shape[0], c_float(short_llr), _np(Lch)),
               "RM_Demodulate_Recover_host")
        return Lch
    rx = _rm_host(rx, (rm.E * m,), np.float32, "rx")
    Lch = np.empty((rx.shape[0], rm.N, q - 1), np.float32)
    _check(lib.nbldpc_rm_demodulate_bpsk_recover_host(rm._h, q, _np(rx), c_float(sigma), rx.shape[0], c_float(short_llr), _np(Lch)),
           "RM_Demodulate_Recover_host")
    return Lch


def RM_Demodulate_Combine_host(rm, q, rx, sigma, L_acc, done=None, short_llr=1.0e4, CONSTELLATION=None):
    """The host statement of RM_Demodulate_Combine: Demodulate_host at N := E, then RM_Combine_host (L_acc updated in place)."""
    q, m = _q_of(q)
    acc = _rm_acc_host(L_acc, rm.N, q - 1)
    B = acc.shape[0]
    done = _rm_done_host(done, B)
    dp = None if done is None else _np(done)
    if CONSTELLATION is not None:
        rx, con = _rm_host(rx, (rm.E, 2), np.float32, "rx", B), _rm_con(CONSTELLATION, q)
        _check(lib.nbldpc_rm_demodulate_qam_combine_host(rm._h, q, _np(rx), _np(con), c_float(sigma), B, c_float(short_llr), dp, _np(acc)),
               "RM_Demodulate_Combine_host")
        return acc
    rx = _rm_host(rx, (rm.E * m,), np.float32, "rx", B)
    _check(lib.nbldpc_rm_demodulate_bpsk_combine_host(rm._h, q, _np(rx), c_float(sigma), B, c_float(short_llr), dp, _np(acc)),
           "RM_Demodulate_Combine_host")
    return acc


def Demodulate_NQ(N, q, rx, sigma, stream=None, CONSTELLATION=None):
    """Demodulate without a code object (nbldpc_demodulate_*_nq): N symbols of GF(q), e.g. the E transmitted symbols of a profile."""
    q, m = _q_of(q)
    if CONSTELLATION is not None:
        B, dev = _rm_dev(rx, (N, 2), torch.float32, "rx")
        Lch = torch.empty((B, N, q - 1), dtype=torch.float32, device=dev)
        _check(lib.nbldpc_demodulate_qam_nq(N, q, _dev(rx), _dev(_rm_con(CONSTELLATION, q, dev)), c_float(sigma), B, _dev(Lch), _stream(stream, dev)),
               "Demodulate_NQ")
        return Lch
    B, dev = _rm_dev(rx, (N * m,), torch.float32, "rx")
    Lch = torch.empty((B, N, q - 1), dtype=torch.float32, device=dev)
    _check(lib.nbldpc_demodulate_bpsk_nq(N, q, _dev(rx), c_float(sigma), B, _dev(Lch), _stream(stream, dev)), "Demodulate_NQ")
    return Lch


def Demodulate_NQ_host(N, q, rx, sigma, CONSTELLATION=None):
    """nbldpc_demodulate_*_nq_host: the demodulators' expressions on host arrays, no device needed."""
    q, m = _q_of(q)
    if CONSTELLATION is not None:
        rx, con = _rm_host(rx, (N, 2), np.float32, "rx"), _rm_con(CONSTELLATION, q)
        Lch = np.empty((rx.shape[0], N, q - 1), np.float32)
        _check(lib.nbldpc_demodulate_qam_nq_host(N, q, _np(rx), _np(con), c_float(sigma), rx.shape[0], _np(Lch)), "Demodulate_NQ_host")
        return Lch
    rx = _rm_host(rx, (N * m,), np.float32, "rx")
    Lch = np.empty((rx.shape[0], N, q - 1), np.float32)
    _check(lib.nbldpc_demodulate_bpsk_nq_host(N, q, _np(rx), c_float(sigma), rx.shape[0], _np(Lch)), "Demodulate_NQ_host")
    return Lch


def RM_Force_Shortened_host(rm, info_pos, msg):
    """nbldpc_rm_force_shortened_host: the forcing step of PN_CodeWords(rate_match=rm) on a host array msg int32 [B, K'] (a copy is
    returned): message symbol k becomes 0 where info_pos[k] is a shortened position."""
    info = np.ascontiguousarray(info_pos, np.int32).reshape(-1)
    msg = _rm_host(msg, (info.size,), np.int32, "msg").copy()
    _check(lib.nbldpc_rm_force_shortened_host(rm._h, _np(info), info.size, msg.shape[0], _np(msg)), "RM_Force_Shortened_host")
    return msg


def AWGNChannel_RM_GPU(seed, sigma, rm, q, tx_sym, stream=None):
    """nbldpc_awgn_channel_device_frames at N := E: tx_sym CUDA int32 [B, E] (RM_Select) -> rx CUDA float32 [B, E*m] over BPSK.
    seed (int32[3]) advances by 4 E m B draws."""
    if not (isinstance(seed, np.ndarray) and seed.dtype == np.int32 and seed.size == 3):
        raise ValueError("seed must be an int32 numpy array of 3")
    q, m = _q_of(q)
    B, dev = _rm_dev(tx_sym, (rm.E,), torch.int32, "tx_sym")
    rx = torch.empty((B, rm.E * m), dtype=torch.float32, device=dev)
    _check(lib.nbldpc_awgn_channel_device_frames(_np(seed), c_float(sigma), _dev(tx_sym), rm.E, m, B, _dev(rx), _stream(stream, dev)), "AWGNChannel_RM_GPU")
    return rx
