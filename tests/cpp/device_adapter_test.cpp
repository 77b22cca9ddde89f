// device_adapter_test.cpp -- include/lccrf_densecrf_gpu.hpp against include/lccrf_densecrf.hpp on the same problem:
//   1. DenseCRFGPU<2> with two PottsPotentialGPU terms (device features, device labels, device confidences) against DenseCRFHIP<2>
//      on host arrays: Q and labels bit-identical, whole inference and stepwise;
//   2. a FOREIGN potential on device arrays (written here: out += c * in) between two PottsPotentialGPU terms -- the CRF steps
//      through the base class's virtuals on device arrays -- against the same mix through DenseCRFHIP with the host twin of that
//      potential: the same bits;
//   3. PottsPotentialGPU::apply on its own (a private one-term CRF) against PottsPotentialHIP::apply.
//   device_adapter_test <in.bin>     in: int32 N; float conf; float fa[N][2], fs[N][2]; float w1, w2; int16 label[N]
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "lccrf_densecrf_gpu.hpp"

using namespace DenseCRF;
using namespace std;

static void hip_ok(hipError_t e, const char *what)
{
    if (e != hipSuccess) throw runtime_error(string(what) + ": " + hipGetErrorString(e));
}

// somebody else's pairwise term on host arrays: out += c * in
class ScaledIdentity : public PairwisePotential {
    int M_;
    float c_;
public:
    ScaledIdentity(int N, int M, float c) : PairwisePotential(N), M_(M), c_(c) {}
    void apply(float *out, const float *in, float *) const override
    {
        for (size_t k = 0; k < (size_t)N_ * M_; ++k) out[k] += c_ * in[k];
    }
};

// ... and its twin on device arrays (synchronous copies: finished when apply() returns, as DenseCRFGPU asks of a foreign term)
class ScaledIdentityGPU : public PairwisePotential {
    int M_;
    float c_;
public:
    ScaledIdentityGPU(int N, int M, float c) : PairwisePotential(N), M_(M), c_(c) {}
    void apply(float *out, const float *in, float *) const override
    {
        const size_t n = (size_t)N_ * M_;
        vector<float> o(n), i(n);
        hip_ok(hipMemcpy(o.data(), out, n * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy");
        hip_ok(hipMemcpy(i.data(), in, n * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy");
        for (size_t k = 0; k < n; ++k) o[k] += c_ * i[k];
        hip_ok(hipMemcpy(out, o.data(), n * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
    }
};

template <class T>
static T *to_device(const vector<T> &v)
{
    T *p = nullptr;
    hip_ok(hipMalloc(&p, sizeof(T) * (v.size() + 1)), "hipMalloc");
    if (!v.empty()) hip_ok(hipMemcpy(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice), "hipMemcpy");
    return p;
}

template <class T>
static vector<T> to_host(const T *p, size_t n)
{
    vector<T> v(n);
    if (n) hip_ok(hipMemcpy(v.data(), p, sizeof(T) * n, hipMemcpyDeviceToHost), "hipMemcpy");
    return v;
}

static int differ(const float *a, const float *b, size_t n) { return n && memcmp(a, b, n * sizeof(float)) != 0; }

int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    int N = 0;
    float conf = 0, w1 = 0, w2 = 0;
    if (fread(&N, 4, 1, fp) != 1 || fread(&conf, 4, 1, fp) != 1) return 2;
    constexpr int M = 2;
    vector<float> fa((size_t)N * 2), fs((size_t)N * 2);
    vector<short> label(N);
    if (fread(fa.data(), 4, fa.size(), fp) != fa.size() || fread(fs.data(), 4, fs.size(), fp) != fs.size() ||
        fread(&w1, 4, 1, fp) != 1 || fread(&w2, 4, 1, fp) != 1 || fread(label.data(), 2, N, fp) != (size_t)N)
        return 2;
    fclose(fp);
    const size_t NM = (size_t)N * M;
    int bad = 0;
    try {
        float *d_fa = to_device(fa), *d_fs = to_device(fs);
        short *d_label = to_device(label);
        float *d_conf = to_device(vector<float>(M, conf));
        // ---- 1. all terms ours ------------------------------------------------------------------
        {
            DenseCRFHIP<M> ref(N);
            ref.setUnaryEnergyFromLabel(label.data(), conf);
            ref.addPairwiseEnergy(new PottsPotentialHIP<M, 2>(fa.data(), N, w1));
            ref.addPairwiseEnergy(new PottsPotentialHIP<M, 2>(fs.data(), N, w2));
            ref.inference(5, true);
            DenseCRFGPU<M> crf(N);
            crf.setUnaryEnergyFromLabel(d_label, d_conf);           // device confidences, as the README's interface has them
            crf.addPairwiseEnergy(new PottsPotentialGPU<M, 2>(d_fa, N, w1));
            crf.addPairwiseEnergy(new PottsPotentialGPU<M, 2>(d_fs, N, w2));
            crf.inference(5, true);
            int b = crf.mixed() || differ(to_host(crf.getProbability(), NM).data(), ref.getProbability(), NM) ||
                    to_host(crf.getMap(), N) != vector<short>(ref.getMap(), ref.getMap() + N);
            crf.startInference();                                     // stepwise
            crf.stepInference();
            ref.startInference();
            ref.stepInference();
            b += differ(to_host(crf.getProbability(), NM).data(), ref.getProbability(), NM);
            bad += b;
            printf("device terms: %s\n", b ? "MISMATCH" : "ok");
        }
        // ---- 2. a foreign device potential between two of ours ------------------------------------------
        {
            DenseCRFHIP<M> ref(N);
            ref.setUnaryEnergyFromLabel(label.data(), conf);
            ref.addPairwiseEnergy(new PottsPotentialHIP<M, 2>(fa.data(), N, w1));
            ref.addPairwiseEnergy(new ScaledIdentity(N, M, 0.25f));
            ref.addPairwiseEnergy(new PottsPotentialHIP<M, 2>(fs.data(), N, w2));
            ref.inference(5, true);
            DenseCRFGPU<M> crf(N);
            crf.setUnaryEnergyFromLabel(d_label, conf);
            crf.addPairwiseEnergy(new PottsPotentialGPU<M, 2>(d_fa, N, w1));
            crf.addPairwiseEnergy(new ScaledIdentityGPU(N, M, 0.25f));
            crf.addPairwiseEnergy(new PottsPotentialGPU<M, 2>(d_fs, N, w2));
            crf.inference(5, true);
            int b = !crf.mixed() || !ref.mixed() || differ(to_host(crf.getProbability(), NM).data(), ref.getProbability(), NM) ||
                    to_host(crf.getMap(), N) != vector<short>(ref.getMap(), ref.getMap() + N);
            bad += b;
            printf("foreign device potential: %s\n", b ? "MISMATCH" : "ok");
        }
        // ---- 3. apply() on its own ----------------------------------------------------------------------
        {
            vector<float> in(NM), out(NM), tmp(NM);
            for (size_t i = 0; i < NM; ++i) {
                in[i] = (float)((i * 2654435761u) % 1000) / 1000.0f;
                out[i] = (float)((i * 40503u) % 97) / 10.0f - 4.0f;
            }
            float *d_in = to_device(in), *d_out = to_device(out), *d_tmp = to_device(tmp);
            PottsPotentialHIP<M, 2> host_pot(fs.data(), N, w2);
            host_pot.apply(out.data(), in.data(), tmp.data());
            PottsPotentialGPU<M, 2> dev_pot(d_fs, N, w2);
            const PairwisePotential &base = dev_pot;
            base.apply(d_out, d_in, d_tmp);
            const int b = differ(to_host(d_out, NM).data(), out.data(), NM);
            bad += b;
            printf("stand-alone apply: %s\n", b ? "MISMATCH" : "ok");
            (void)hipFree(d_in);
            (void)hipFree(d_out);
            (void)hipFree(d_tmp);
        }
        (void)hipFree(d_fa);
        (void)hipFree(d_fs);
        (void)hipFree(d_label);
        (void)hipFree(d_conf);
    } catch (const std::exception &e) {
        fprintf(stderr, "device_adapter_test: %s\n", e.what());
        return 1;
    }
    if (bad) return 1;
    printf("DEVICE ADAPTER OK\n");
    return 0;
}
