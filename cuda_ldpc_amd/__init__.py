"""cuda_ldpc_amd -- MI355X-native LDPC belief-propagation decoders.

Python host-side mirror of the reference's entry points (gsw4869/CUDA_LDPC) over
the C ABI in include/*.h.  The compute lives in libcuda_ldpc_amd.so (hand-written
HIP for gfx950); PyTorch is used only for device memory, streams and
torch.distributed.  There is no CPU fallback: importing the decoders without
the built extension raises.
"""
from . import _lib  # noqa: F401
from .bldpc import (BinaryCode, Get_H, Transform_H, LDPC_Decoder_GPU, Decode_Statistic, Statistic, SimCounters, AWGNChannel_CPU, AWGNChannel_GPU, sigma_of,  # noqa: F401
                    Encode, PN_CodeWords, Syndrome, generator_host, pn_messages, LDPC_Decoder_Layered_GPU, layered_host, normalised_host,
                    LDPC_Decoder_BP_GPU, bp_host, BP_Table, Quant, LDPC_Decoder_Quant_GPU, quant_host,
                    Modulate_QAM, AWGNChannel_QAM_GPU, Demodulate_QAM, Modulate_QAM_host, Demodulate_QAM_host, Get_CONSTELLATION, qc_variants, qc_plan_host,
                    RateMatch, RM_Select, RM_Recover, AWGNChannel_RM_GPU, RM_Select_host, RM_Recover_host, AWGNChannel_RM_CPU,
                    RM_Combine, AWGNChannel_RM_Combine_GPU, Frames_Gather, Frames_Scatter, RM_Combine_host, AWGNChannel_RM_Combine_CPU,
                    Frames_Gather_host, Frames_Scatter_host, RM_Modulate_QAM, RM_Demodulate_QAM_Recover, RM_Demodulate_QAM_Combine,
                    RM_Modulate_QAM_host, RM_Demodulate_QAM_Recover_host, RM_Demodulate_QAM_Combine_host, IL_NONE, IL_ROWCOL,
                    Fading, QUASI_STATIC, Fading_Gains, Fading_Gains_host, AWGNChannel_Fading_GPU, AWGNChannel_Fading_CPU,
                    AWGNChannel_QAM_Fading_GPU, AWGNChannel_QAM_Fading_CPU, Demodulate_QAM_Fading, Demodulate_QAM_Fading_host,
                    BF_THRESHOLD, BF_GRADIENT, Hard_Pack, Hard_Pack_Int, Hard_Unpack, Hard_Pack_host, Hard_Pack_Int_host, Hard_Unpack_host, BSCChannel_GPU, BSCChannel_CPU, LDPC_Decoder_BitFlip_GPU, bitflip_host, bitflip_plan_host,
                    BECChannel_GPU, BECChannel_CPU, LDPC_Decoder_Erasure_GPU, erasure_host, erasure_plan_host, RM_Select_Bits, RM_Recover_Bits, RM_Select_Bits_host, RM_Recover_Bits_host, Statistic_Bits, Statistic_Bits_host,
                    LDPC_Decoder_Erasure_ML_GPU, erasure_ml_host, erasure_ml_plan_host, ML_NONE, ML_SOLVED, ML_PARTIAL, ML_STUCK, ML_INCONSISTENT, ML_SKIPPED,
                    LDPC_Decoder_OSD_GPU, osd_host, osd_plan_host,
                    STOP_PREFIX, STOP_SYNDROME, EXIT_FIXED, EXIT_BATCH_GLOBAL, EXIT_PER_FRAME, KERNEL_AUTO, KERNEL_TABLE, KERNEL_QC_LDS)

__all__ = ["BinaryCode", "Get_H", "Transform_H", "LDPC_Decoder_GPU", "Decode_Statistic", "Statistic", "SimCounters", "AWGNChannel_CPU", "AWGNChannel_GPU", "sigma_of",
           "Encode", "PN_CodeWords", "Syndrome", "generator_host", "pn_messages", "LDPC_Decoder_Layered_GPU", "layered_host", "normalised_host",
           "LDPC_Decoder_BP_GPU", "bp_host", "BP_Table", "Quant", "LDPC_Decoder_Quant_GPU", "quant_host",
           "Modulate_QAM", "AWGNChannel_QAM_GPU", "Demodulate_QAM", "Modulate_QAM_host", "Demodulate_QAM_host", "Get_CONSTELLATION", "qc_variants", "qc_plan_host",
           "RateMatch", "RM_Select", "RM_Recover", "AWGNChannel_RM_GPU", "RM_Select_host", "RM_Recover_host", "AWGNChannel_RM_CPU",
           "RM_Combine", "AWGNChannel_RM_Combine_GPU", "Frames_Gather", "Frames_Scatter", "RM_Combine_host", "AWGNChannel_RM_Combine_CPU",
           "Frames_Gather_host", "Frames_Scatter_host", "RM_Modulate_QAM", "RM_Demodulate_QAM_Recover", "RM_Demodulate_QAM_Combine",
           "RM_Modulate_QAM_host", "RM_Demodulate_QAM_Recover_host", "RM_Demodulate_QAM_Combine_host", "IL_NONE", "IL_ROWCOL",
           "Fading", "QUASI_STATIC", "Fading_Gains", "Fading_Gains_host", "AWGNChannel_Fading_GPU", "AWGNChannel_Fading_CPU",
           "AWGNChannel_QAM_Fading_GPU", "AWGNChannel_QAM_Fading_CPU", "Demodulate_QAM_Fading", "Demodulate_QAM_Fading_host",
           "BF_THRESHOLD", "BF_GRADIENT", "Hard_Pack", "Hard_Pack_Int", "Hard_Unpack", "Hard_Pack_host", "Hard_Pack_Int_host", "Hard_Unpack_host", "BSCChannel_GPU", "BSCChannel_CPU", "LDPC_Decoder_BitFlip_GPU", "bitflip_host", "bitflip_plan_host",
           "BECChannel_GPU", "BECChannel_CPU", "LDPC_Decoder_Erasure_GPU", "erasure_host", "erasure_plan_host", "RM_Select_Bits", "RM_Recover_Bits", "RM_Select_Bits_host", "RM_Recover_Bits_host", "Statistic_Bits", "Statistic_Bits_host",
           "LDPC_Decoder_Erasure_ML_GPU", "erasure_ml_host", "erasure_ml_plan_host", "ML_NONE", "ML_SOLVED", "ML_PARTIAL", "ML_STUCK", "ML_INCONSISTENT", "ML_SKIPPED",
           "LDPC_Decoder_OSD_GPU", "osd_host", "osd_plan_host",
           "STOP_PREFIX", "STOP_SYNDROME",
           "EXIT_FIXED", "EXIT_BATCH_GLOBAL", "EXIT_PER_FRAME", "KERNEL_AUTO", "KERNEL_TABLE", "KERNEL_QC_LDS"]
