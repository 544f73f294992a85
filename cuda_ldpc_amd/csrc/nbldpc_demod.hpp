// nbldpc_demod.hpp -- the two per-element expressions of Demodulate (src/LDPC_Decoder.cpp:139-169), written once: the demodulator
// kernels of nbldpc_channel.hip, the fused rate-matching kernels of nbldpc_ratematch.hip and the host statements of nbldpc_rm_host.hpp
// all call these, so "the fused call is the demodulator followed by recover / combine, bit for bit" holds by construction.  The build
// compiles with -ffp-contract=off; the pragma keeps a stand-alone host program that forgot the flag to the same bits.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CLDPC_HD __host__ __device__
#else
#define CLDPC_HD
#endif

namespace cldpc {

// BPSK branch: L_ch[k-1] of one symbol from its m received bits r[0..m), element k in 1..q-1.
CLDPC_HD inline float nb_demod_bpsk_entry(const float *r, int k, int m, float sigma)
{
#pragma clang fp contract(off)
    const float s2 = sigma * sigma;
    float acc = 0.0f;
    for (int b = 0; b < m; b++)
        if ((k & (1 << b)) != 0) acc += (float)(-2) * r[b] / s2;
    return acc;
}

// n_QAM != 2 branch: L_ch[k-1] of one symbol from its received point (yr, yi), the point of element 0 (c0r, c0i) and the point of
// element k (ckr, cki), float arithmetic in the reference's order.
CLDPC_HD inline float nb_demod_qam_entry(float yr, float yi, float c0r, float c0i, float ckr, float cki, float sigma)
{
#pragma clang fp contract(off)
    return ((2 * yr - c0r - ckr) * (ckr - c0r) + (2 * yi - c0i - cki) * (cki - c0i)) / (2 * sigma * sigma);
}

} // namespace cldpc
