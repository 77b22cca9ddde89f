// csrc/fused_loop.h's host-callable plan functions, printed for tests/test_chain_rows.py.  One query per line of standard input:
//   T                                 -> "T chain_top_rank(0) ... chain_top_rank(63)"
//   L NA K V0 V1 row0 nt limit        -> "L ok chain0 prod_all total Ecap0 Ecap1 chain_wanted"       (layout_core; limit in bytes)
//   P NA V len_0 .. len_{V-1}         -> "P slack aligned end Ecap": rows of these lengths in vertex order, row[v] their prefix sums;
//                                        slack = min over v < V - 1 of pst(row[v+1], v+1) - pst(row[v], v) - len_v, aligned = every
//                                        start and every step a multiple of 4, end = pst(row[V-1], V-1) + ceil4(len_{V-1}) + 8,
//                                        Ecap = plane_floats(NA, V, true)
//   C                                 -> "C kChainTop kChainMinRow kChainGap chain_max_v(1024) chain_max_v(512) kLdsLimit kLdsHalf"
#include "fused_loop.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

int main()
{
    using namespace lccrf::fl;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char what = 0;
        in >> what;
        if (what == 'T') {
            printf("T");
            for (int ln = 0; ln < 64; ++ln) printf(" %d", chain_top_rank(ln));
            printf("\n");
        } else if (what == 'L') {
            int NA = 0, K = 0, V[2] = {0, 0}, row0 = 0, nt = 0;
            long limit = 0;
            in >> NA >> K >> V[0] >> V[1] >> row0 >> nt >> limit;
            FusedLayout lay{};
            const bool ok = layout_core(NA, K, V, row0, &lay, nt, (size_t)limit);
            printf("L %d %d %d %d %d %d %d\n", ok ? 1 : 0, lay.chain0, lay.prod_all, lay.total, lay.Ecap[0], lay.Ecap[1],
                   chain_wanted(NA, V[0], row0, nt) ? 1 : 0);
        } else if (what == 'P') {
            int NA = 0, V = 0;
            in >> NA >> V;
            std::vector<int> len(V), row(V + 1, 0);
            for (int v = 0; v < V; ++v) {
                in >> len[v];
                row[v + 1] = row[v] + len[v];
            }
            int slack = 1 << 30, aligned = 1;
            for (int v = 0; v < V; ++v) {
                const int a = pst(row[v], v);
                if (a & 3) aligned = 0;
                if (v + 1 < V) {
                    const int step = pst(row[v + 1], v + 1) - a;
                    if (step & 3) aligned = 0;
                    if (step - len[v] < slack) slack = step - len[v];
                }
            }
            const int end = V ? pst(row[V - 1], V - 1) + ((len[V - 1] + 3) & ~3) + 8 : 0;
            printf("P %d %d %d %d\n", slack, aligned, end, plane_floats(NA, V, true));
        } else if (what == 'C') {
            printf("C %d %d %d %d %d %d %d\n", kChainTop, kChainMinRow, kChainGap, chain_max_v(kNT), chain_max_v(kNTSmall), (int)kLdsLimit,
                   (int)kLdsHalf);
        }
    }
    return 0;
}
