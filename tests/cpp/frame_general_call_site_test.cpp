// frame_general_call_site_test.cpp -- the tracker's sequence (src/Tracking.cc:1919-1930: construct, unaries from labels, two
// potentials, infer once, read the labels) through DenseCRFHIP<2> with a learnt model -- a label-compatibility matrix on the appearance
// potential, the SYMMETRIC normalisation on the smoothness potential -- and LCCRF_OPT_FRAME_GENERAL set: runConverged builds both
// lattices, normalises and infers until the labels settle in ONE launch (csrc/frame_general.hip).
//
//   frame_general_call_site_test <inputs.bin> <outputs.bin>
//       inputs:  int32 N, float obs[N], float err[N], float xy[2N], int16 label[N], float mu[4]
//       outputs: float Q[2N], int16 label[N], int32 engine, int32 iterations, int32 changed, int32 converged, float delta
//
// The numbers are checked by tests/test_frame_general.py against the oracle's float32 restatement; the engine is reported here and
// checked there.  Exit 0 when the program ran, 3 when the library reports that no GPU is usable (the adapter throws -- no fallback).
#include <cstdio>
#include <cstring>
#include <vector>

#include "lccrf_densecrf.hpp"

struct Point2f { float x, y; };
struct Point3f { float x, y, z; };

using namespace DenseCRF;
using namespace std;

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    int N = 0;
    if (fread(&N, 4, 1, fp) != 1 || N < 0) return 2;
    const size_t n = (size_t)N;
    vector<float> vobservs(n), verrors(n);
    vector<Point2f> vcorrd2d(n);
    vector<Point3f> vpoints(n);
    vector<short> init_label(n);
    float mu[4];
    if (fread(vobservs.data(), 4, n, fp) != n || fread(verrors.data(), 4, n, fp) != n || fread(vcorrd2d.data(), 8, n, fp) != n ||
        fread(init_label.data(), 2, n, fp) != n || fread(mu, 4, 4, fp) != 4)
        return 2;
    fclose(fp);
    FILE *fo = fopen(argv[2], "wb");
    if (!fo) return 2;

    // TUM3.yaml:78-101
    const float mConf = 0.7f, mW1 = 10.0f, mW2 = 30.0f, mObservStdev = 1.5f, mRpjErrorStdev = 0.6f, mPoint3dStdev = 0.5f,
                mPoint2dStdev = 18.0f;
    const int M = 2;
    try {
        DenseCRFHIP<M> crf(N);
        crf.setOption(LCCRF_OPT_FRAME_GENERAL, 1);
        crf.setUnaryEnergyFromLabel(init_label.data(), mConf);

        auto *appearancePairwise = PottsPotentialHIP<M, 2>::appearanceKernel(N, mW1, vobservs, verrors, mObservStdev, mRpjErrorStdev);
        appearancePairwise->setCompatibility(mu);
        crf.addPairwiseEnergy(appearancePairwise);

        auto *smoothnessPairwise = PottsPotentialHIP<M, 2>::smoothKernel(N, mW2, vpoints, vcorrd2d, mPoint3dStdev, mPoint2dStdev);
        crf.addPairwiseEnergy(smoothnessPairwise);
        smoothnessPairwise->setNormalization(LCCRF_NORMALIZE_SYMMETRIC);

        crf.runConverged(12, LCCRF_STOP_LABELS, 0.0f, true);
        short *res_label = crf.getMap();
        const int engine = crf.engine(), iterations = crf.iterations(), changed = crf.changed(), converged = crf.converged() ? 1 : 0;
        const float delta = crf.delta();
        fwrite(crf.getProbability(), 4, 2 * n, fo);
        fwrite(res_label, 2, n, fo);
        fwrite(&engine, 4, 1, fo);
        fwrite(&iterations, 4, 1, fo);
        fwrite(&changed, 4, 1, fo);
        fwrite(&converged, 4, 1, fo);
        fwrite(&delta, 4, 1, fo);
        fclose(fo);
        printf("FRAME GENERAL CALL-SITE DONE N=%d engine=%d iterations=%d converged=%d\n", N, engine, iterations, converged);
        return 0;
    } catch (const std::exception &e) {
        printf("EXCEPTION: %s\n", e.what());
        return strstr(e.what(), "no HIP device") ? 3 : 4;
    }
}
