// prints lean_sorted_vertex (csrc/fused_lean.h) for the vertex counts given on the command line: "V q number" per line
#include "fused_lean.h"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    for (int i = 1; i < argc; ++i) {
        const int V = atoi(argv[i]);
        for (int q = 0; q < V; ++q) printf("%d %d %d\n", V, q, lccrf::fl::lean_sorted_vertex(q, V, lccrf::fl::kNTSmall));
    }
    return 0;
}
