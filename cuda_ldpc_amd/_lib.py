"""Loader of libcuda_ldpc_amd.so (the C ABI declared in include/bldpc.h, include/nbldpc.h)."""
import ctypes
import os

import torch  # noqa: F401  -- first, so that ONE HIP runtime (torch's) serves the whole process

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("CUDA_LDPC_AMD_SO") or os.path.join(_HERE, "libcuda_ldpc_amd.so")  # env: experiments only


class ExtensionMissing(ImportError):
    pass


def load():
    if not os.path.exists(SO_PATH):
        raise ExtensionMissing(
            "%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
            "There is no CPU fallback." % SO_PATH)
    return ctypes.CDLL(SO_PATH)


lib = load()

c_int, c_void_p, c_char_p = ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p
lib.bldpc_last_error.restype = c_char_p
lib.bldpc_last_kernel.restype = c_char_p
lib.bldpc_last_kernel.argtypes = [c_void_p]
lib.bldpc_qc_variant_count.argtypes = []
lib.bldpc_qc_variant_info.argtypes = [c_int, c_void_p, ctypes.POINTER(c_char_p)]
lib.bldpc_code_qc_info.argtypes = [c_void_p, c_void_p]
lib.bldpc_qc_plan_host.argtypes = [c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p]
lib.bldpc_read_blockh.argtypes = [c_char_p, c_int, c_int, c_void_p, c_void_p, c_void_p]
lib.bldpc_transform_h.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int]
lib.bldpc_code_create_qc.argtypes = [c_int, c_int, c_int, c_void_p, ctypes.POINTER(c_void_p)]
lib.bldpc_code_create_table.argtypes = [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_void_p)]
lib.bldpc_code_destroy.argtypes = [c_void_p]
lib.bldpc_code_dims.argtypes = [c_void_p, c_void_p]
lib.bldpc_decode.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                             ctypes.POINTER(c_int), c_void_p]
lib.bldpc_decode_per_frame.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
lib.bldpc_statistic.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]
lib.bldpc_statistic_per_frame.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]
lib.bldpc_decode_statistic.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
lib.bldpc_set_profiling.argtypes = [c_void_p, c_int]
lib.bldpc_last_kernel_ms.argtypes = [c_void_p, ctypes.POINTER(ctypes.c_float)]
lib.bldpc_kernel_ms_mean.argtypes = [c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(c_int)]
lib.bldpc_awgn_channel_host.argtypes = [c_void_p, ctypes.c_float, c_void_p, c_void_p, c_int, c_int]
lib.bldpc_awgn_channel_device.argtypes = [c_void_p, ctypes.c_float, c_void_p, c_void_p, c_int, c_int, c_void_p]
lib.bldpc_generator_host.argtypes = [c_int, c_int, c_int, c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_void_p, c_void_p]
lib.bldpc_encoder_info.argtypes = [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int), c_void_p]
lib.bldpc_encode.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p]
lib.bldpc_encode_random.argtypes = [c_void_p, ctypes.c_ulonglong, ctypes.c_longlong, c_int, c_void_p, c_void_p, c_void_p]
lib.bldpc_syndrome.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]
lib.bldpc_decode_layered.argtypes = [c_void_p, c_void_p, c_int, c_int, ctypes.c_float, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
lib.bldpc_decode_layered_host.argtypes = [c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, ctypes.c_float, c_int, c_int, c_int, c_void_p,
                                          c_void_p, c_void_p]
lib.bldpc_decode_layered_bp.argtypes = [c_void_p, c_void_p, c_int, c_int, ctypes.c_float, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
lib.bldpc_decode_layered_bp_host.argtypes = [c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, ctypes.c_float, c_int, c_int, c_int, c_void_p,
                                             c_void_p, c_void_p]
lib.bldpc_bp_table.argtypes = [c_void_p]


class bldpc_quant(ctypes.Structure):
    """struct bldpc_quant of include/bldpc.h, unchecked: cuda_ldpc_amd.Quant is the checked one."""
    _fields_ = [("llr_scale", ctypes.c_float), ("bits_ch", c_int), ("bits_app", c_int), ("bits_msg", c_int), ("norm8", c_int), ("offset", c_int)]


lib.bldpc_decode_layered_quant.argtypes = [c_void_p, c_void_p, c_int, c_int, ctypes.POINTER(bldpc_quant), c_int, c_int, c_int, c_void_p, c_void_p,
                                           c_void_p, c_void_p]
lib.bldpc_decode_layered_quant_host.argtypes = [c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, ctypes.POINTER(bldpc_quant), c_int, c_int, c_int,
                                                c_void_p, c_void_p, c_void_p]
lib.bldpc_decode_normalised.argtypes = [c_void_p, c_void_p, c_int, c_int, ctypes.c_float, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
lib.bldpc_decode_normalised_host.argtypes = [c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, ctypes.c_float, c_int, c_int, c_void_p, c_void_p,
                                             c_void_p]
lib.bldpc_qam_map.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]
lib.bldpc_qam_demap.argtypes = [c_void_p, c_void_p, c_int, ctypes.c_float, c_int, c_int, c_void_p, c_void_p]
lib.bldpc_qam_map_host.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p]
lib.bldpc_qam_demap_host.argtypes = [c_void_p, c_void_p, c_int, ctypes.c_float, c_int, c_int, c_void_p]
lib.bldpc_qam_map_il.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]
lib.bldpc_qam_demap_il.argtypes = [c_void_p, c_void_p, c_int, ctypes.c_float, c_int, c_int, c_int, c_void_p, c_void_p]
lib.bldpc_qam_map_il_host.argtypes = [c_void_p, c_int, c_int, c_int, c_int, c_void_p]
lib.bldpc_qam_demap_il_host.argtypes = [c_void_p, c_void_p, c_int, ctypes.c_float, c_int, c_int, c_int, c_void_p]
lib.bldpc_rm_qam_map.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]
lib.bldpc_rm_qam_recover.argtypes = [c_void_p, c_void_p, c_void_p, c_int, ctypes.c_float, c_int, c_int, ctypes.c_float, c_void_p, c_void_p]
lib.bldpc_rm_qam_combine.argtypes = [c_void_p, c_void_p, c_void_p, c_int, ctypes.c_float, c_int, c_int, ctypes.c_float, c_void_p, c_void_p, c_void_p]
lib.bldpc_rm_qam_map_host.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]
lib.bldpc_rm_qam_recover_host.argtypes = [c_void_p, c_void_p, c_void_p, c_int, ctypes.c_float, c_int, c_int, ctypes.c_float, c_void_p]
lib.bldpc_rm_qam_combine_host.argtypes = [c_void_p, c_void_p, c_void_p, c_int, ctypes.c_float, c_int, c_int, ctypes.c_float, c_void_p, c_void_p]
lib.bldpc_rm_create.argtypes =[c_int, c_void_p, c_int, c_void_p, c_int, ctypes.POINTER(c_void_p)]
lib.bldpc_rm_destroy.argtypes = [c_void_p]
lib.bldpc_rm_dims.argtypes = [c_void_p, c_void_p]
lib.bldpc_rm_tx_pos.argtypes = [c_void_p, c_void_p]
lib.bldpc_rm_select.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p]
lib.bldpc_rm_recover.argtypes = [c_void_p, c_void_p, c_int, ctypes.c_float, c_void_p, c_void_p]
lib.bldpc_rm_awgn_channel_device.argtypes = [c_void_p, c_void_p, ctypes.c_float, c_void_p, c_int, ctypes.c_float, c_void_p, c_void_p]
lib.bldpc_rm_select_host.argtypes = [c_void_p, c_void_p, c_int, c_void_p]
lib.bldpc_rm_recover_host.argtypes = [c_void_p, c_void_p, c_int, ctypes.c_float, c_void_p]
lib.bldpc_rm_awgn_channel_host.argtypes = [c_void_p, c_void_p, ctypes.c_float, c_void_p, c_int, ctypes.c_float, c_void_p]
lib.bldpc_rm_encode_random.argtypes = [c_void_p, c_void_p, ctypes.c_ulonglong, ctypes.c_longlong, c_int, c_void_p, c_void_p, c_void_p]
lib.bldpc_rm_create_circular.argtypes = [c_int, c_void_p, c_int, c_void_p, c_int, c_int, c_int, ctypes.POINTER(c_void_p)]
lib.bldpc_rm_circ.argtypes = [c_void_p, c_void_p]
lib.bldpc_rm_combine.argtypes = [c_void_p, c_void_p, c_int, ctypes.c_float, c_void_p, c_void_p, c_void_p]
lib.bldpc_rm_awgn_combine_device.argtypes = [c_void_p, c_void_p, ctypes.c_float, c_void_p, c_int, ctypes.c_float, c_void_p, c_void_p, c_void_p]
lib.bldpc_rm_combine_host.argtypes = [c_void_p, c_void_p, c_int, ctypes.c_float, c_void_p, c_void_p]
lib.bldpc_rm_awgn_combine_host.argtypes = [c_void_p, c_void_p, ctypes.c_float, c_void_p, c_int, ctypes.c_float, c_void_p, c_void_p]
lib.bldpc_frames_gather.argtypes = [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]
lib.bldpc_frames_scatter.argtypes = [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]
lib.bldpc_frames_gather_host.argtypes = [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p]
lib.bldpc_frames_scatter_host.argtypes = [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p]
lib.bldpc_fading_gains_device.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]
lib.bldpc_fading_gains_host.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p]
lib.bldpc_awgn_fading_channel_device.argtypes = [c_void_p, ctypes.c_float, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]
lib.bldpc_awgn_fading_channel_host.argtypes = [c_void_p, ctypes.c_float, c_void_p, c_void_p, c_void_p, c_int, c_int]
lib.bldpc_qam_demap_fading.argtypes = [c_void_p, c_void_p, c_void_p, c_int, ctypes.c_float, c_int, c_int, c_int, c_void_p, c_void_p]
lib.bldpc_qam_demap_fading_host.argtypes = [c_void_p, c_void_p, c_void_p, c_int, ctypes.c_float, c_int, c_int, c_int, c_void_p]
lib.nbldpc_fading_channel_device_qam_frames.argtypes = [c_void_p, ctypes.c_float, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]
lib.nbldpc_fading_channel_host_qam_frames.argtypes = [c_void_p, ctypes.c_float, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p]
lib.nbldpc_demodulate_qam_fading.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_float, c_int, c_void_p, c_void_p]
lib.nbldpc_demodulate_qam_fading_nq.argtypes = [c_int, c_int, c_void_p, c_void_p, c_void_p, ctypes.c_float, c_int, c_void_p, c_void_p]
lib.nbldpc_demodulate_qam_fading_host.argtypes = [c_int, c_int, c_void_p, c_void_p, c_void_p, ctypes.c_float, c_int, c_void_p]
lib.bldpc_hard_pack.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p]
lib.bldpc_hard_pack_int.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p]
lib.bldpc_hard_unpack.argtypes = [c_void_p, c_int, c_int, c_void_p, c_void_p]
lib.bldpc_hard_pack_host.argtypes = [c_void_p, c_int, c_int, c_void_p]
lib.bldpc_hard_pack_int_host.argtypes = [c_void_p, c_int, c_int, c_void_p]
lib.bldpc_hard_unpack_host.argtypes = [c_void_p, c_int, c_int, c_void_p]
lib.bldpc_bsc_channel_device.argtypes = [c_void_p, ctypes.c_float, c_void_p, c_int, c_int, c_void_p, c_void_p]
lib.bldpc_bsc_channel_host.argtypes = [c_void_p, ctypes.c_float, c_void_p, c_int, c_int, c_void_p]
lib.bldpc_decode_bitflip.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
lib.bldpc_decode_bitflip_host.argtypes = [c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]
lib.bldpc_bitflip_info.argtypes = [c_void_p, c_void_p]
lib.bldpc_bitflip_plan_host.argtypes = [c_int, c_int, c_int, c_void_p, c_void_p]
lib.bldpc_bec_channel_device.argtypes = [c_void_p, ctypes.c_float, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]
lib.bldpc_bec_channel_host.argtypes = [c_void_p, ctypes.c_float, c_void_p, c_int, c_int, c_void_p, c_void_p]
lib.bldpc_decode_erasure.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
lib.bldpc_decode_erasure_host.argtypes = [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
lib.bldpc_erasure_info.argtypes = [c_void_p, c_void_p]
lib.bldpc_erasure_plan_host.argtypes = [c_int, c_int, c_int, c_void_p, c_void_p]
lib.bldpc_decode_erasure_ml.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
lib.bldpc_decode_erasure_ml_host.argtypes = [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p]
lib.bldpc_erasure_ml_info.argtypes = [c_void_p, c_int, c_int, c_void_p]
lib.bldpc_erasure_ml_plan_host.argtypes = [c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p]
lib.bldpc_decode_osd.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
lib.bldpc_decode_osd_host.argtypes = [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]
lib.bldpc_osd_info.argtypes = [c_void_p, c_int, c_void_p]
lib.bldpc_osd_plan_host.argtypes = [c_int, c_int, c_int, c_void_p, c_int, c_void_p]
lib.bldpc_decode_osd_w.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
lib.bldpc_decode_osd_w_host.argtypes = [c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p]
lib.bldpc_osd_w_info.argtypes = [c_void_p, c_int, c_int, c_void_p]
lib.bldpc_osd_w_plan_host.argtypes = [c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p]
lib.bldpc_rm_select_bits.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_void_p]
lib.bldpc_rm_recover_bits.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]
lib.bldpc_rm_select_bits_host.argtypes = [c_void_p, c_void_p, c_int, c_void_p]
lib.bldpc_rm_recover_bits_host.argtypes = [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]
lib.bldpc_statistic_bits.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]
lib.bldpc_statistic_bits_host.argtypes = [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p]
lib.bldpc_sigma.restype = ctypes.c_float
lib.bldpc_sigma.argtypes = [ctypes.c_float, c_int, ctypes.c_float]


class LdpcError(RuntimeError):
    pass


def check(rc, what):
    if rc != 0:
        raise LdpcError("%s failed (%d): %s" % (what, rc, lib.bldpc_last_error().decode(errors="replace")))
