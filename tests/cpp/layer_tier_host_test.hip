// layer_tier_host_test.hip -- the tier rules of the three row-layered decoders (choose_tier of csrc/bldpc_layered_host.hpp,
// bldpc_bp_host.hpp and bldpc_quant_host.hpp, all over layer::choose_tier of csrc/bldpc_layer_host.hpp) as a stand-alone program, to be
// built with the address + undefined sanitizers.  No HIP call, no kernel launch, no GPU.
// Reads lines "J Z N M EZ" (M check rows, EZ edges of one frame) and prints per line, for min-sum, sum-product and quantised min-sum
// in turn, "kernel units threads lds regj": what bldpc_last_kernel would name, units per workgroup (0 = the workspace kernel), threads,
// dynamic LDS bytes, and J of the register variant (min-sum only, otherwise 0).  tests/test_layered_cpu.py compares the lines with
// tests/golden/layer_tier_choices.json.
#include <cstdio>
#include "../../cuda_ldpc_amd/csrc/bldpc_bp_host.hpp"
#include "../../cuda_ldpc_amd/csrc/bldpc_layered_host.hpp"
#include "../../cuda_ldpc_amd/csrc/bldpc_quant_host.hpp"

using namespace cldpc;

int main()
{
    int J, Z, N, M, EZ, n = 0;
    while (scanf("%d %d %d %d %d", &J, &Z, &N, &M, &EZ) == 5) {
        const layh::Tier a = layh::choose_tier(J, Z, N, M);
        const layer::Tier b = bph::choose_tier(Z, N, EZ), c = qh::choose_tier(J, Z, N);
        printf("%s %d %d %d %d %s %d %d %d 0 %s %d %d %d 0\n", !a.units ? "k_lay_ws" : a.regj ? "k_lay_reg" : "k_lay", a.units, a.threads, a.lds,
               a.regj, b.units ? "k_lbp" : "k_lbp_ws", b.units, b.threads, b.lds, c.units ? "k_lq" : "k_lq_ws", c.units, c.threads, c.lds);
        n++;
    }
    printf("OK %d\n", n);
    return 0;
}
