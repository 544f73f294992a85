// nbldpc_qspa_ws.hpp -- the sizes both tiers of the FHT sum-product decoders are built from (the LDS bound, the vectors of a workgroup,
// the bytes of a frame's state) and the plan of the workspace tier (k_nb_qspa_ws / k_nb_qspa_ws_layered, nbldpc_qspa_kernel.hpp):
// threads per workgroup, LDS bytes and workspace-slot bytes of a code, or a refusal.  Host only, no HIP call and no device code:
// tests/cpp/nb_qspa_ws_plan_host_test.hip compiles it alone; the constexpr functions are what the kernels call as well.
//
// The layout the numbers come from.  A frame's vectors: p [N][q] floats, then the message vectors [M][dc][q] floats.  Fixed part: the
// decisions [N] and 4 flag words as ints, TableMultiply as bytes [q][q].  LDS tier: the vectors, then the fixed part, all in LDS.
// Workspace tier: the vectors in a workspace slot (global memory, one per resident workgroup); in LDS the fixed part and NV row slabs
// of dc * q floats, one per vector of lanes.
#pragma once
#include <cstddef>

namespace cldpc {

constexpr size_t kQspaMaxLds = 159 * 1024;         // the LDS one workgroup of either tier may use
constexpr size_t kQspaWsMaxBytes = (size_t)2 << 30; // the most workspace one call allocates
constexpr int kQspaWsMaxSlots = 1024;
constexpr int kQspaWsSizes[5] = {1024, 512, 256, 128, 64};

struct QspaWsPlan {
    int threads = 0, vectors = 0; // vectors: NV, the row slabs
    size_t lds_bytes = 0, slot_bytes = 0;
    const char *why = ""; // the refusal, where threads == 0
};

inline bool qspa_ws_size_ok(int nt)
{
    for (int s : kQspaWsSizes)
        if (s == nt) return true;
    return false;
}

// NV, the vectors of q entries a workgroup holds at a time: W = min(q, 64) lanes each (nbldpc_qspa_kernel.hpp)
constexpr int qspa_vectors(int threads, int q) { return threads / 64 * (q < 64 ? 64 / q : 1); }

constexpr size_t qspa_ws_fixed_lds(int N, int q) { return ((size_t)N + 4) * 4 + (size_t)q * q; }

inline size_t qspa_ws_lds_bytes(int N, int q, int dc, int threads)
{
    return qspa_ws_fixed_lds(N, q) + (size_t)4 * qspa_vectors(threads, q) * dc * q;
}

constexpr size_t qspa_ws_slot_bytes(int N, int M, int q, int dc) { return ((size_t)N * q + (size_t)M * dc * q) * 4; }

// The LDS of the LDS tier: a frame's vectors and the fixed part.
constexpr size_t qspa_lds_bytes(int N, int M, int q, int dc) { return qspa_ws_slot_bytes(N, M, q, dc) + qspa_ws_fixed_lds(N, q); }

// The rule.  The largest of 1024 ... 64 threads whose LDS total is at most 159 KiB: phases A and C, the syndrome and every copy use
// all the vectors there are.  Layered: the row sweep can use no more vectors than a level has rows, so if a smaller size among those
// that fit already holds the widest level in one pass, the smallest such size.  pin: NBLDPC_QSPA_WS_THREADS, 0 = the rule.
// threads == 0 in the result: refused, and why.
inline QspaWsPlan qspa_ws_plan(int N, int M, int q, int dc, int widest_level, bool layered, int pin = 0)
{
    QspaWsPlan pl;
    int m = 0;
    while ((1 << m) < q) m++;
    if (N <= 0 || M <= 0 || dc <= 0) { pl.why = "N, M and dcmax must be positive"; return pl; }
    if (q < 4 || q > 256 || (1 << m) != q) { pl.why = "q must be a power of two with 4 <= q <= 256"; return pl; }
    if (pin && !qspa_ws_size_ok(pin)) { pl.why = "the pinned workgroup size is not one of 64, 128, 256, 512, 1024"; return pl; }
    const size_t slot = qspa_ws_slot_bytes(N, M, q, dc);
    if (slot >= kQspaWsMaxBytes) { pl.why = "one workspace slot does not fit in 2 GiB"; return pl; }
    int nt = 0;
    if (pin) {
        if (qspa_ws_lds_bytes(N, q, dc, pin) > kQspaMaxLds) { pl.why = "the pinned workgroup size needs more than 159 KiB of LDS"; return pl; }
        nt = pin;
    } else {
        for (int s : kQspaWsSizes) { // descending
            if (qspa_ws_lds_bytes(N, q, dc, s) > kQspaMaxLds) continue;
            if (!nt) nt = s;
            if (layered && qspa_vectors(s, q) >= widest_level) nt = s; // ends at the smallest that holds the widest level
        }
        if (!nt) { pl.why = "the decisions, TableMultiply and one wave's row slabs exceed 159 KiB of LDS"; return pl; }
    }
    pl.threads = nt;
    pl.vectors = qspa_vectors(nt, q);
    pl.lds_bytes = qspa_ws_lds_bytes(N, q, dc, nt);
    pl.slot_bytes = slot;
    return pl;
}

// Slots of one call: min(B, 1024, what fits in 2 GiB, the cap of NBLDPC_QSPA_WS_SLOTS (0 = none)), at least 1.
inline int qspa_ws_slots(int B, size_t slot_bytes, int cap)
{
    size_t n = (size_t)(B < kQspaWsMaxSlots ? B : kQspaWsMaxSlots);
    const size_t fit = kQspaWsMaxBytes / slot_bytes;
    if (fit < n) n = fit;
    if (cap > 0 && (size_t)cap < n) n = (size_t)cap;
    return n < 1 ? 1 : (int)n;
}

} // namespace cldpc
