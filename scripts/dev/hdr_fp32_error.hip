// Development measurement (not part of the product): the error, in texels, of the FP32 texel coordinate that background()'s HDR branch
// (raytracer_project_amd/csrc/zr_device.h) trusts away from texel boundaries, with the device's own atan2f / acosf, against long double.
// The number behind that branch's comment and its guard of 0.02 texel.
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=fast hdr_fp32_error.hip -o hdr_fp32_error && ./hdr_fp32_error
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

// the coordinate exactly as background() forms it
__global__ void coords(const double* d, size_t n, float width, float height, float* out) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float xf = (float)d[3 * k], yf = (float)d[3 * k + 1], zf = (float)d[3 * k + 2];
    const float PIf = 3.14159265358979323846f;
    out[2 * k] = (atan2f(zf, xf) + PIf) * (0.15915494309189535f * width);
    out[2 * k + 1] = acosf(fminf(fmaxf(yf, -1.0f), 1.0f)) * (0.3183098861837907f * height);
}

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static double u01() {   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}
#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

int main() {
    const size_t n = 4u << 20;
    const long double PI = 3.14159265358979323846;   // the double constant, as in the reference
    std::vector<double> d(3 * n);
    std::vector<float> got(2 * n);
    double* dd; float* dout;
    HIP_OK(hipMalloc(&dd, d.size() * sizeof(double))); HIP_OK(hipMalloc(&dout, got.size() * sizeof(float)));
    for (int size : {64, 1024, 4096, 16384}) {
        // unit directions with |y| < 0.999 (the branch's own condition): half uniform in (phi, theta), half aimed at 0.02 texel from a boundary of a size-texel axis
        for (size_t k = 0; k < n; k++) {
            long double fu = u01() * size, fv = u01() * size;
            if (k & 1) { if (k & 2) fu = std::floor(fu) + (k & 4 ? 0.02L : 0.98L); else fv = std::floor(fv) + (k & 4 ? 0.02L : 0.98L); }
            const long double phi = fu / size * 2 * PI - PI, th = fv / size * PI;
            d[3 * k] = (double)(std::sin(th) * std::cos(phi)); d[3 * k + 1] = (double)std::cos(th); d[3 * k + 2] = (double)(std::sin(th) * std::sin(phi));
        }
        HIP_OK(hipMemcpy(dd, d.data(), d.size() * sizeof(double), hipMemcpyHostToDevice));
        coords<<<dim3((unsigned)((n + 255) / 256)), dim3(256)>>>(dd, n, (float)size, (float)size, dout);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(got.data(), dout, got.size() * sizeof(float), hipMemcpyDeviceToHost));
        long double eu = 0, ev = 0; size_t used = 0;
        for (size_t k = 0; k < n; k++) {
            const long double x = d[3 * k], y = d[3 * k + 1], z = d[3 * k + 2];
            if (std::fabs((float)y) >= 0.999f) continue;
            used++;
            const long double ru = (std::atan2(z, x) + PI) / (2 * PI) * size, rv = std::acos(y) / PI * size;
            eu = std::fmax(eu, std::fabs((long double)got[2 * k] - ru)); ev = std::fmax(ev, std::fabs((long double)got[2 * k + 1] - rv));
        }
        std::printf("%5d texels: max error of the FP32 coordinate over %zu directions: u %.5f texel, v %.5f texel\n", size, used, (double)eu, (double)ev);
    }
    HIP_OK(hipFree(dd)); HIP_OK(hipFree(dout));
    return 0;
}
