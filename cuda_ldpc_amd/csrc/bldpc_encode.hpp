// bldpc_encode.hpp -- what bldpc_encode.hip (encoder, syndrome) needs from the code object of bldpc_api.hip.
#pragma once

struct bldpc_code;

namespace cldpc {

struct EncState; // generator + device tables of one code object, built on first use (bldpc_encode.hip)

struct CodeView {
    int J, L, Z, N, M, K;
    const int *H;   // block shifts [J*L] (host), nullptr for a code built from an address table
    EncState **enc; // the code object's slot for its EncState
};

CodeView code_view(const bldpc_code *c); // bldpc_api.hip
void enc_state_free(EncState *s);        // bldpc_encode.hip

} // namespace cldpc
