// run_converged_call_site_test.cpp -- the tracker's sequence (src/Tracking.cc:1919-1930: construct, unaries, two pairwise terms,
// infer, read the labels; a fresh CRF per frame) with inference(5, true) replaced by runConverged(10, LCCRF_STOP_LABELS, ...)
// (include/lccrf.h section 1i: the whole frame in one launch), written against the drop-in adapter include/lccrf_densecrf.hpp and
// checked against the oracle's C API stepped by hand with the contract's definitions.
//
//   run_converged_call_site_test <inputs.bin>     inputs: int32 N, float obs[N], float err[N], float xy[2N], int16 label[N]
//
// Exit 0 and print "RUN CONVERGED OK ..." when the iteration count, delta's bits, the flip count, the labels and Q's bits are the
// oracle's and the engine is the one-launch one (3), for LABELS and for DELTA.  Exit 3 when the library reports that no GPU is
// usable (the adapter throws -- no fallback).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lccrf_densecrf.hpp"
#include "../../oracle/lccrf_oracle.h"      // the CHECKER; tests may link it, the product never does

struct Point2f { float x, y; };
struct Point3f { float x, y, z; };

using namespace DenseCRF;
using namespace std;

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    int N = 0;
    if (fread(&N, 4, 1, fp) != 1) return 2;
    vector<float> vobservs(N), verrors(N);
    vector<Point2f> vcorrd2d(N);
    vector<Point3f> vpoints(N);
    vector<short> init_label(N);
    if (fread(vobservs.data(), 4, N, fp) != (size_t)N || fread(verrors.data(), 4, N, fp) != (size_t)N ||
        fread(vcorrd2d.data(), 8, N, fp) != (size_t)N || fread(init_label.data(), 2, N, fp) != (size_t)N)
        return 2;
    fclose(fp);

    // TUM3.yaml:78-101
    const float mConf = 0.7f, mW1 = 10.0f, mW2 = 30.0f, mObservStdev = 1.5f, mRpjErrorStdev = 0.6f,
                mPoint3dStdev = 0.5f, mPoint2dStdev = 18.0f;
    const int M = 2, kCap = 10;

    try {
        orc_crf *o = orc_crf_create(N, M);
        float conf[M] = {mConf, mConf};
        orc_crf_set_unary_from_label(o, init_label.data(), conf);
        vector<float> f((size_t)2 * N + 1);
        orc_appearance_features(N, vobservs.data(), verrors.data(), mObservStdev, mRpjErrorStdev, f.data());
        orc_crf_add_pairwise(o, f.data(), 2, mW1);
        orc_smooth_features(N, &vcorrd2d[0].x, mPoint2dStdev, f.data());
        orc_crf_add_pairwise(o, f.data(), 2, mW2);

        int bad = 0;
        const int criteria[2] = {LCCRF_STOP_LABELS, LCCRF_STOP_DELTA};
        const float tols[2] = {0.0f, 1e-2f};
        for (int c = 0; c < 2; ++c) {
            // ---- the call site: one frame, one CRF --------------------------------------------------
            DenseCRFHIP<M> crf(N);
            crf.setUnaryEnergyFromLabel(init_label.data(), mConf);
            crf.addPairwiseEnergy(PottsPotentialHIP<M, 2>::appearanceKernel(N, mW1, vobservs, verrors, mObservStdev, mRpjErrorStdev));
            crf.addPairwiseEnergy(PottsPotentialHIP<M, 2>::smoothKernel(N, mW2, vpoints, vcorrd2d, mPoint3dStdev, mPoint2dStdev));
            crf.runConverged(kCap, criteria[c], tols[c], true);
            short *res_label = crf.getMap();
            // ---------------------------------------------------------------------------------------
            // the oracle, stepped by hand: d_t and c_t by the definitions of section 1h
            orc_crf_start_inference(o);
            vector<float> prev((size_t)N * M);
            int t = 0, changed = 0, met = 0;
            float delta = 0.0f;
            while (t < kCap && !met) {
                memcpy(prev.data(), o->current, sizeof(float) * prev.size());
                orc_crf_step_inference(o, 1.0f);
                ++t;
                delta = 0.0f;
                changed = 0;
                for (int i = 0; i < N; ++i) {
                    for (int l = 0; l < M; ++l) delta = fmaxf(delta, fabsf(o->current[i * M + l] - prev[i * M + l]));
                    changed += (o->current[i * M] < o->current[i * M + 1]) != (prev[i * M] < prev[i * M + 1]);
                }
                met = (!(criteria[c] & LCCRF_STOP_DELTA) || delta <= tols[c]) && (!(criteria[c] & LCCRF_STOP_LABELS) || changed == 0);
            }
            orc_crf_build_map(o);
            int bad_label = 0;
            for (int i = 0; i < N; ++i) bad_label += res_label[i] != o->map[i];
            const float got_delta = crf.delta();
            const int bad_q = memcmp(crf.getProbability(), o->current, sizeof(float) * (size_t)N * M) != 0;
            const int bad_report = crf.iterations() != t || memcmp(&got_delta, &delta, 4) != 0 || crf.changed() != changed ||
                                   crf.converged() != (met != 0);
            printf("criterion %d: iterations %d (oracle %d) delta %.9g (%.9g) changed %d (%d) converged %d (%d) label_mismatches=%d "
                   "q_bit_identical=%d engine=%d\n", criteria[c], crf.iterations(), t, got_delta, delta, crf.changed(), changed,
                   (int)crf.converged(), met, bad_label, !bad_q, crf.engine());
            bad += bad_label || bad_q || bad_report || crf.engine() != 3;
        }
        orc_crf_destroy(o);
        printf("%s N=%d\n", bad ? "RUN CONVERGED MISMATCH" : "RUN CONVERGED OK", N);
        return bad ? 1 : 0;
    } catch (const std::exception &e) {
        printf("EXCEPTION: %s\n", e.what());
        return strstr(e.what(), "no HIP device") ? 3 : 4;
    }
}
