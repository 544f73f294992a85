// bldpc_ratematch.hpp -- what bldpc_ratematch.hip (shortening, puncturing) and bldpc_encode.hip share.
#pragma once

struct bldpc_code;
struct bldpc_rm;

namespace cldpc {

// What bldpc_modem.hip reads of a profile for the fused modem calls ("rate matching over QAM" in include/bldpc.h).  d_map [N] and
// d_tx [E] are the profile's device tables; they stay NULL unless rm_view was asked to upload them.  map, tx_pos and short_pos
// [n_short] are the host tables, owned by the profile (nbldpc_ratematch.hip: the GF(q) half reads a profile over symbols through them).
struct RmView {
    int N, E, Ncb, k0, laps, n_short, n_punct;
    const int *d_map, *d_tx;
    const int *map, *tx_pos, *short_pos;
};
// bldpc_ratematch.hip: device = true uploads the tables on first use, as every device call on a profile does (BLDPC_ENOMEM / _EHIP)
int rm_view(const bldpc_rm *rm, bool device, RmView *v);

// The profile's one table, int [N]: the rank b >= 0 of a position in the buffer (the positions neither shortened nor punctured,
// ascending; a linear profile transmits them in this order, so b is its e), or one of these.
constexpr int kRmPunct = -1, kRmShort = -2;

// bldpc_encode.hip: bldpc_encode_random with every message bit whose information position is marked kRmShort in d_map (device
// int [N]) forced to 0.  short_pos (host, ascending) is checked against the generator's information set before anything is launched.
int encode_random_shortened(bldpc_code *code, const int *d_map, const int *short_pos, int n_short, unsigned long long seed,
                            long long first_frame, int F, int *msg, int *cw, void *stream);

} // namespace cldpc
