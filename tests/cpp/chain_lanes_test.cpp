// prints lean_chain_row (csrc/fused_lean.h) for every lane of a 512-lane workgroup, "L lane rank label" (rank -1: no row), and
// lean_chain_waves for every vertex count of the plan, "W V0 wavefronts"; with arguments NA V1 (points per frame, vertices of the
// smoothness lattice) also "P <the most appearance-lattice vertices with which layout_lean fits half a CU's LDS>"
#include "fused_lean.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    using namespace lccrf::fl;
    for (int t = 0; t < kNTSmall; ++t) {
        const int cr = lean_chain_row(t);
        printf("L %d %d %d\n", t, cr < 0 ? -1 : (cr & 0xffff), cr < 0 ? -1 : (cr >> 16));
    }
    for (int V0 = 0; V0 <= chain_max_v(kNTSmall); ++V0) printf("W %d %d\n", V0, lean_chain_waves(V0));
    printf("T %d %d\n", kLeanChainTop, chain_max_v(kNTSmall));
    if (argc > 2) {
        FusedLayout lay;
        int V[2] = {chain_max_v(kNTSmall), atoi(argv[2])};
        while (V[0] > 0 && !layout_lean(atoi(argv[1]), 2, V, kChainMinRow, &lay, kNTSmall, kLdsHalf)) --V[0];
        printf("P %d\n", V[0]);
    }
    return 0;
}
