// image_demo_gpu_test.cpp -- the README's GPU sequence (Thirdparty/DenseCRF/README.md, "GPU Version") against
// include/lccrf_densecrf_gpu.hpp: DenseCRFGPU<21>, labels and image in device memory, the two image potentials built by
// PottsPotentialGPU<21, F>::FromImage on the device, getMap() a device pointer read back with hipMemcpy.  The image runs twice,
// as a float image (FromImage<float>, the README's call) and as the uint8 image itself (FromImage<unsigned char>).  The Python
// test colours both label sets and compares them with the reference's known answer (res1_cpu.ppm).
//   image_demo_gpu_test <in.bin> <out.bin>    in: int32 W, H; uint8 rgb[W*H*3]; int16 anno[W*H]    out: int16 map[2][W*H] (float, uint8)
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <vector>

#include "lccrf_densecrf_gpu.hpp"

using namespace DenseCRF;
using namespace std;

#define HIP_OK(x)                                                                   \
    do {                                                                            \
        if ((x) != hipSuccess) {                                                    \
            fprintf(stderr, "image_demo_gpu_test: %s failed\n", #x);                \
            return 1;                                                               \
        }                                                                           \
    } while (0)

template <class T>
static int run(int W, int H, const short *labelGPU, const T *rgbGPU, short *map_host)
{
    const int N = W * H, M = 21;
    DenseCRFGPU<M> crf(N);
    crf.setUnaryEnergyFromLabel(labelGPU, 0.5);
    crf.addPairwiseEnergy(PottsPotentialGPU<M, 2>::FromImage<>(W, H, 3.0, 3.0));
    crf.addPairwiseEnergy(PottsPotentialGPU<M, 5>::template FromImage<T>(W, H, 10.0, 60.0, rgbGPU, 20.0));
    crf.inference(10, true);
    short *mapGPU = crf.getMap();
    HIP_OK(hipMemcpy(map_host, mapGPU, sizeof(short) * N, hipMemcpyDeviceToHost));
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) return 2;
    int W = 0, H = 0;
    if (fread(&W, 4, 1, fp) != 1 || fread(&H, 4, 1, fp) != 1) return 2;
    const int N = W * H;
    vector<unsigned char> im((size_t)N * 3);
    vector<short> anno(N);
    if (fread(im.data(), 1, im.size(), fp) != im.size() || fread(anno.data(), 2, N, fp) != (size_t)N) return 2;
    fclose(fp);
    vector<float> imf(im.begin(), im.end());
    vector<short> maps((size_t)2 * N);
    short *labelGPU = nullptr;
    unsigned char *rgbGPU = nullptr;
    float *rgbFeatGPU = nullptr;
    HIP_OK(hipMalloc(&labelGPU, sizeof(short) * N));
    HIP_OK(hipMalloc(&rgbGPU, im.size()));
    HIP_OK(hipMalloc(&rgbFeatGPU, sizeof(float) * imf.size()));
    HIP_OK(hipMemcpy(labelGPU, anno.data(), sizeof(short) * N, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(rgbGPU, im.data(), im.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(rgbFeatGPU, imf.data(), sizeof(float) * imf.size(), hipMemcpyHostToDevice));
    int rc = 0;
    try {
        rc = run<float>(W, H, labelGPU, rgbFeatGPU, maps.data());
        if (!rc) rc = run<unsigned char>(W, H, labelGPU, rgbGPU, maps.data() + N);
    } catch (const std::exception &e) {
        fprintf(stderr, "image_demo_gpu_test: %s\n", e.what());
        rc = 1;
    }
    (void)hipFree(labelGPU);
    (void)hipFree(rgbGPU);
    (void)hipFree(rgbFeatGPU);
    if (rc) return rc;
    FILE *fo = fopen(argv[2], "wb");
    if (!fo || fwrite(maps.data(), 2, maps.size(), fo) != maps.size()) return 2;
    fclose(fo);
    printf("IMAGE DEMO GPU OK\n");
    return 0;
}
