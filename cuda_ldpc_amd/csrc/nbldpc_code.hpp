// nbldpc_code.hpp -- the GF(q) code object behind include/nbldpc.h.  Built and freed by nbldpc_api.hip (nbldpc_code_create, in the
// stages of nbldpc_plan.hpp); nbldpc_channel.hip reads its dimensions, nbldpc_encode.hip goes through nb_code_view.
#pragma once
#include <atomic>
#include <vector>

#include "nbldpc_encode.hpp"

struct nbldpc_code {
    int N = 0, M = 0, q = 0, m = 0, dv = 0, dc = 0;
    int *d_vn_w = nullptr, *d_vn_thr = nullptr, *d_vn_gf = nullptr;
    int *d_cn_w = nullptr, *d_cn_src = nullptr, *d_cn_gf = nullptr, *d_cn_vn = nullptr;
    unsigned char *d_mul = nullptr;
    size_t lds_bytes = 0;
    // trellis min-max decoders (nbldpc_tmm_decode_batch)
    int *d_cn_hinv = nullptr, *d_row_order = nullptr, *d_level_begin = nullptr;
    int levels = 0;
    bool tmm_ok = false;
    int qspa_layered_threads = 0; // k_nb_qspa_layered: threads per workgroup (256 / 512 / 1024), fixed at create time
    bool row_repeats = false;     // a row lists one variable in two slots: refused by nbldpc_qspa_layered_decode_batch
    int widest_level = 0;         // the most rows any dependency level holds: the layered plan of the workspace tier (nbldpc_qspa_ws.hpp)
    int qspa_ws_threads = 0, qspa_ws_slots = 0; // NBLDPC_QSPA_WS_THREADS / NBLDPC_QSPA_WS_SLOTS, read once at create time (0: the plan's rule / no cap)
    int zero_coeff = 0; // an edge with coefficient 0 exists (EMS only, see nb_tables_build)
    const char *last_kernel = "none"; // nbldpc_last_kernel
    int persist_grid = 0; // k_nb_ems / k_nb_ems_wide: workgroups that fill the chip once (CUs x workgroups per CU)
    bool hbm = false;   // decoded by k_nb_ems_hbm (state in a global-memory workspace): LDS too small or rows heavier than kNbMaxW
    int pipe_grid = 0;        // k_nb_ems2 (two frames in flight per workgroup): resident workgroups, 0 = kernel not offered for this code
    size_t pipe_lds = 0;
    int tmm_grid[2] = {0, 0}; // k_nb_tmm<q, layered>: the same, per schedule (0 = flooding, 1 = layered), fixed at create time
    bool no_persist = false;  // NBLDPC_NO_PERSIST, read once at create time (tests / experiments): one workgroup per frame
    // Frame counters of the persistent kernels: a ring of kWorkSlots words, one per decode call in flight (the call zeroes its
    // slot stream-ordered before the launch), instead of a hipMallocAsync / hipFreeAsync pair per call.  Calls on different
    // streams never share a slot unless more than kWorkSlots calls on this code object are in flight at once.
    int *d_work = nullptr;
    std::atomic<unsigned> work_next{0};
    // encoder (nbldpc_encode.hip): host copies of the CN lists and of TableMultiply, and the generator built on first use
    std::vector<int> h_cn_w, h_cn_vn, h_cn_gf;
    std::vector<unsigned> h_mul;
    cldpc::NbEncState *enc = nullptr;
};
