// bldpc_ratematch.hpp -- what bldpc_ratematch.hip (shortening, puncturing) and bldpc_encode.hip share.
#pragma once

struct bldpc_code;

namespace cldpc {

// The profile's one table, int [N]: the rank b >= 0 of a position in the buffer (the positions neither shortened nor punctured,
// ascending; a linear profile transmits them in this order, so b is its e), or one of these.
constexpr int kRmPunct = -1, kRmShort = -2;

// bldpc_encode.hip: bldpc_encode_random with every message bit whose information position is marked kRmShort in d_map (device
// int [N]) forced to 0.  short_pos (host, ascending) is checked against the generator's information set before anything is launched.
int encode_random_shortened(bldpc_code *code, const int *d_map, const int *short_pos, int n_short, unsigned long long seed,
                            long long first_frame, int F, int *msg, int *cw, void *stream);

} // namespace cldpc
