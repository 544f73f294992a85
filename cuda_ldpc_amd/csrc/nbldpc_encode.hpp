// nbldpc_encode.hpp -- what nbldpc_encode.hip (GF(q) encoder, syndrome) needs from the code object of nbldpc_api.hip.
#pragma once

struct nbldpc_code;

namespace cldpc {

struct NbEncState; // generator + device tables of one code object, built on first use (nbldpc_encode.hip)

struct NbCodeView {
    int N, M, q, m, dc;
    const int *cn_w, *cn_vn, *cn_gf;       // host copies of the CN lists ([M], [M][dc], [M][dc])
    const unsigned *mul;                   // host copy of TableMultiply [q][q]
    const int *d_cn_w, *d_cn_vn, *d_cn_gf; // the same on the device
    const unsigned char *d_mul;            // TableMultiply on the device, bytes [q][q]
    NbEncState **enc;                      // the code object's slot for its NbEncState
};

NbCodeView nb_code_view(const nbldpc_code *c); // nbldpc_api.hip
void nb_enc_state_free(NbEncState *s);         // nbldpc_encode.hip

// nbldpc_encode.hip: the information set of the code's generator (built on first use, as nbldpc_encoder_info does): K', info_pos on
// the host and on the device, both owned by the code object.  For nbldpc_ratematch.hip (nbldpc_rm_encode_random).
int nb_enc_info(nbldpc_code *code, const char *who, int *K_info, const int **info_pos, const int **d_info_pos);

} // namespace cldpc
