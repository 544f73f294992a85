// nbldpc_rm_host.hpp -- the host statements of rate matching over GF(q) symbol vectors (include/nbldpc.h, "rate matching"): plain C++
// that follows the words of the header literally, no HIP call, no device code.  nbldpc_ratematch.hip wraps them into the _host entry
// points; tests/cpp/nb_rm_host_test.hip compiles them on their own under the host sanitizers.
//
// A profile is read as its tables: map[n] = the rank of position n in the buffer, kRmPunct or kRmShort (bldpc_ratematch.hpp), and
// tx_pos[e].  Position n of rank r is sent at e_0 = (r - k0) mod Ncb and again at e_0 + Ncb, e_0 + 2 Ncb, ... < E.
#pragma once
#include <cstddef>
#include <cstring>

#include "nbldpc_demod.hpp"

namespace cldpc {
namespace nbrm {

constexpr int kPunct = -1, kShort = -2; // kRmPunct, kRmShort

struct Profile {
    int N, E, Ncb, k0;
    const int *map, *tx_pos; // [N], [E]
};

// tx_sym[b][e] = CodeWord_sym[b][tx_pos[e]]
inline void select_host(const Profile &p, const int *cw, int B, int *tx)
{
    for (int b = 0; b < B; b++)
        for (int e = 0; e < p.E; e++) tx[(size_t)b * p.E + e] = cw[(size_t)b * p.N + p.tx_pos[e]];
}

// recover (acc = L_ch, combine false, done ignored) and combine (acc = L_acc) in one loop, entry by entry.
inline void receive_host(const Profile &p, int V, const float *Lrx, int B, float short_llr, const int *done, float *acc, bool combine)
{
    const float neg = -short_llr;
    for (int b = 0; b < B; b++) {
        if (combine && done && done[b]) continue; // every bit of the frame stays
        for (int n = 0; n < p.N; n++) {
            const int r = p.map[n];
            float *v = acc + ((size_t)b * p.N + n) * V;
            if (r == kShort) {
                for (int k = 0; k < V; k++) v[k] = neg;
                continue;
            }
            const int e0 = r < 0 ? p.E : (r - p.k0 + p.Ncb) % p.Ncb;
            if (e0 >= p.E) { // punctured, or not reached by this transmission
                if (!combine) memset(v, 0, (size_t)V * sizeof(float));
                continue;
            }
            for (int k = 0; k < V; k++) {
                int e = e0;
                if (!combine) { // the first contribution moves as 32 bits
                    memcpy(v + k, Lrx + ((size_t)b * p.E + e) * V + k, sizeof(float));
                    e += p.Ncb;
                }
                for (; e < p.E; e += p.Ncb) {
                    const float s = v[k] + Lrx[((size_t)b * p.E + e) * V + k];
                    v[k] = s;
                }
            }
        }
    }
}

// nbldpc_demodulate_qam_nq / _bpsk_nq as statements: rx [B][N][2] (con [q][2]) or rx [B][N*m] -> L_ch [B][N][q-1]
inline void demod_qam_host(int N, int q, const float *rx, const float *con, float sigma, int B, float *Lch)
{
    for (size_t bs = 0; bs < (size_t)B * N; bs++)
        for (int k = 1; k < q; k++)
            Lch[bs * (q - 1) + k - 1] = nb_demod_qam_entry(rx[2 * bs], rx[2 * bs + 1], con[0], con[1], con[2 * k], con[2 * k + 1], sigma);
}

inline void demod_bpsk_host(int N, int q, int m, const float *rx, float sigma, int B, float *Lch)
{
    for (size_t bs = 0; bs < (size_t)B * N; bs++)
        for (int k = 1; k < q; k++) Lch[bs * (q - 1) + k - 1] = nb_demod_bpsk_entry(rx + bs * m, k, m, sigma);
}

// The forcing step of nbldpc_rm_encode_random: message symbol k of every frame becomes 0 where info_pos[k] is a shortened position.
inline void force_shortened_host(const int *map, const int *info_pos, int K, int B, int *msg)
{
    for (int b = 0; b < B; b++)
        for (int k = 0; k < K; k++)
            if (map[info_pos[k]] == kShort) msg[(size_t)b * K + k] = 0;
}

} // namespace nbrm
} // namespace cldpc
