// learned_call_site_test.cpp -- the reference's call site (src/Tracking.cc:1919-1930) through DenseCRFHIP<2> with the parts a
// training run fits: a label-compatibility matrix on the appearance potential, set BEFORE addPairwiseEnergy, and the SYMMETRIC
// normalisation on the smoothness potential, set AFTER it (include/lccrf_densecrf.hpp: setCompatibility / setNormalization).
//
//   learned_call_site_test <inputs.bin> <outputs.bin>           the call site
//   learned_call_site_test <inputs.bin> <outputs.bin> apply     a stand-alone apply() of a potential that carries both setters
//       inputs:  int32 N, float obs[N], float err[N], float xy[2N], int16 label[N], float mu[4], float x[2N], float out[2N]
//       outputs: call site -- float Q[2N], int16 label[N], int32 engine, int32 shape;  apply -- float out[2N]
//
// The numbers are checked by tests/test_cpp_learned.py against the float32 restatement.  Exit 0 when the program ran, 3 when the
// library reports that no GPU is usable (the adapter throws -- no fallback).
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
    vector<float> vobservs(n), verrors(n), x(2 * n), out(2 * n);
    vector<Point2f> vcorrd2d(n);
    vector<Point3f> vpoints(n);
    vector<short> init_label(n);
    float mu[4];
    if (fread(vobservs.data(), 4, n, fp) != n || fread(verrors.data(), 4, n, fp) != n || fread(vcorrd2d.data(), 8, n, fp) != n ||
        fread(init_label.data(), 2, n, fp) != n || fread(mu, 4, 4, fp) != 4 || fread(x.data(), 4, 2 * n, fp) != 2 * n ||
        fread(out.data(), 4, 2 * n, fp) != 2 * n)
        return 2;
    fclose(fp);
    FILE *fo = fopen(argv[2], "wb");
    if (!fo) return 2;

    // TUM3.yaml:78-101
    const float mConf = 0.7f, mW1 = 10.0f, mW2 = 30.0f, mObservStdev = 1.5f, mRpjErrorStdev = 0.6f, mPoint3dStdev = 0.5f,
                mPoint2dStdev = 18.0f;
    const int M = 2;
    try {
        if (argc > 3 && !strcmp(argv[3], "apply")) {
            auto *p = PottsPotentialHIP<M, 2>::appearanceKernel(N, mW1, vobservs, verrors, mObservStdev, mRpjErrorStdev);
            p->setCompatibility(mu);
            p->setNormalization(LCCRF_NORMALIZE_SYMMETRIC);
            p->apply(out.data(), x.data(), nullptr);
            delete p;
            fwrite(out.data(), 4, 2 * n, fo);
            fclose(fo);
            printf("LEARNED APPLY DONE N=%d\n", N);
            return 0;
        }
        DenseCRFHIP<M> crf(N);
        crf.setUnaryEnergyFromLabel(init_label.data(), mConf);

        auto *appearancePairwise = PottsPotentialHIP<M, 2>::appearanceKernel(N, mW1, vobservs, verrors, mObservStdev, mRpjErrorStdev);
        appearancePairwise->setCompatibility(mu);                                // before the CRF owns it
        crf.addPairwiseEnergy(appearancePairwise);

        auto *smoothnessPairwise = PottsPotentialHIP<M, 2>::smoothKernel(N, mW2, vpoints, vcorrd2d, mPoint3dStdev, mPoint2dStdev);
        crf.addPairwiseEnergy(smoothnessPairwise);
        smoothnessPairwise->setNormalization(LCCRF_NORMALIZE_SYMMETRIC);         // after

        crf.inference(5, true);
        short *res_label = crf.getMap();
        int shape = 0;
        const int engine = crf.engine(&shape);
        fwrite(crf.getProbability(), 4, 2 * n, fo);
        fwrite(res_label, 2, n, fo);
        fwrite(&engine, 4, 1, fo);
        fwrite(&shape, 4, 1, fo);
        fclose(fo);
        printf("LEARNED CALL-SITE DONE N=%d engine=%d shape=0x%x\n", N, engine, shape);
        return 0;
    } catch (const std::exception &e) {
        printf("EXCEPTION: %s\n", e.what());
        return strstr(e.what(), "no HIP device") ? 3 : 4;
    }
}
