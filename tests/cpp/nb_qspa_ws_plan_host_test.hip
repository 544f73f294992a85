// nb_qspa_ws_plan_host_test.hip -- the plan of the workspace tier of the FHT sum-product decoders (csrc/nbldpc_qspa_ws.hpp) as a
// stand-alone host program: no HIP call, no device.  Sweeps q, N, M, dc (and the layered rule over a set of widest levels), checks the
// plan's own invariants on every point, and prints the FNV-1a 64 digest of all answers, {refused ? 0 : threads, LDS bytes, slot bytes,
// NV} as four ints per point, which tests/test_nb_qspa_ws_cpu.py compares with the library's answers on the same sweep.
// Built by the test with the address and undefined-behaviour sanitizers on the host side.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../cuda_ldpc_amd/csrc/nbldpc_qspa_ws.hpp"

using u64 = unsigned long long;

#define NEED(c)                                                          \
    do {                                                                 \
        if (!(c)) {                                                      \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);      \
            return 1;                                                    \
        }                                                                \
    } while (0)

static u64 fnv(const void *p, size_t n)
{
    u64 h = 0xcbf29ce484222325ull;
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

int main()
{
    using namespace cldpc;
    const int qs[] = {4, 8, 16, 32, 64, 128, 256}, Ns[] = {1, 7, 72, 206, 1000, 9472, 24000, 40000}, dcs[] = {2, 3, 4, 12, 21, 40, 64, 96};
    const int wides[] = {0, 1, 3, 4, 5, 16, 17, 64, 65, 1000};
    std::vector<int> all;
    long points = 0, refused = 0;
    for (int q : qs)
        for (int N : Ns)
            for (int dc : dcs)
                for (int M : {1, N / 2 + 1}) {
                    int last_threads = 0;
                    for (int k = 0; k <= 10; k++) { // k = 0: flooding; k >= 1: layered with wides[k - 1]
                        const bool layered = k > 0;
                        const int wide = layered ? wides[k - 1] : 0;
                        const QspaWsPlan pl = qspa_ws_plan(N, M, q, dc, wide, layered);
                        points++;
                        if (!pl.threads) {
                            refused++;
                            NEED(pl.why && pl.why[0]);
                            NEED(qspa_ws_lds_bytes(N, q, dc, 64) > kQspaMaxLds || qspa_ws_slot_bytes(N, M, q, dc) >= kQspaWsMaxBytes);
                            all.insert(all.end(), {0, 0, 0, 0});
                            continue;
                        }
                        NEED(qspa_ws_size_ok(pl.threads));
                        NEED(pl.lds_bytes == qspa_ws_lds_bytes(N, q, dc, pl.threads) && pl.lds_bytes <= kQspaMaxLds);
                        NEED(pl.vectors == qspa_vectors(pl.threads, q) && pl.slot_bytes == qspa_ws_slot_bytes(N, M, q, dc));
                        if (!layered) {
                            last_threads = pl.threads; // the largest that fits: twice as many threads would not
                            NEED(pl.threads == 1024 || qspa_ws_lds_bytes(N, q, dc, 2 * pl.threads) > kQspaMaxLds);
                        } else {
                            NEED(pl.threads <= last_threads);
                            if (pl.threads < last_threads) NEED(pl.vectors >= wide && (pl.threads == 64 || qspa_vectors(pl.threads / 2, q) < wide));
                            else NEED(pl.vectors < wide || pl.threads == 64 || qspa_vectors(pl.threads / 2, q) < wide);
                        }
                        // a pin gives that size or a refusal, and never changes the slot
                        for (int pin : kQspaWsSizes) {
                            const QspaWsPlan pp = qspa_ws_plan(N, M, q, dc, wide, layered, pin);
                            NEED(pp.threads == (qspa_ws_lds_bytes(N, q, dc, pin) <= kQspaMaxLds ? pin : 0));
                            NEED(!pp.threads || pp.slot_bytes == pl.slot_bytes);
                        }
                        NEED(!qspa_ws_plan(N, M, q, dc, wide, layered, 96).threads);
                        const int slots = qspa_ws_slots(300, pl.slot_bytes, 0);
                        NEED(slots >= 1 && slots <= 300 && (slots == 1 || (size_t)slots * pl.slot_bytes <= kQspaWsMaxBytes));
                        NEED(qspa_ws_slots(300, pl.slot_bytes, 5) <= 5 && qspa_ws_slots(3, pl.slot_bytes, 5) <= 3 && qspa_ws_slots(5000, pl.slot_bytes, 0) <= 1024);
                        all.insert(all.end(), {pl.threads, (int)pl.lds_bytes, (int)pl.slot_bytes, pl.vectors});
                    }
                }
    NEED(!qspa_ws_plan(1, 1, 256, 96, 0, false).threads && !qspa_ws_plan(0, 1, 16, 4, 0, false).threads && !qspa_ws_plan(8, 4, 48, 4, 0, false).threads);
    NEED(!qspa_ws_plan(8, 4, 2, 4, 0, false).threads && !qspa_ws_plan(8, 4, 512, 4, 0, false).threads);
    printf("%ld points, %ld refused\n%016llx\n", points, refused, fnv(all.data(), all.size() * sizeof(int)));
    return 0;
}
