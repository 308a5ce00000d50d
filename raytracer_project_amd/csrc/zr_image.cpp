// zr_image.cpp — the image-space entry points of the C ABI (include/zr_capi.h), which need a context and no scene: the post stack, the two a-trous denoisers
// (the variance-guided one, also behind zr_accum_denoise), the non-local-means denoiser (also behind zr_accum_denoise_nlm), sharpening and the frame analysis.
#include "zr_frame.h"

namespace zr_host {
namespace {

// a frame an image entry accepts: sides of at least min_side, at most 2^31 pixels
int check_frame_size(int W, int H, int min_side) {
    return W < min_side || H < min_side || (size_t)W * H > (1ull << 31) ? fail(ZR_E_INVALID, "frame size %d x %d not supported", W, H) : ZR_OK;
}

// the guide frames of a denoiser, n pixels each, to the device: albedo, normal and, where the caller has one, depth
int upload_guides(zr_ctx* c, const double* albedo, const double* normal, const double* zdepth, size_t n, DevBuf<double>& d_a, DevBuf<double>& d_n, DevBuf<double>& d_z) {
    int rc;
    if ((rc = d_a.alloc(n * 3)) || (rc = d_n.alloc(n * 3)) || (zdepth && (rc = d_z.alloc(n * 3)))) return rc;
    HIP_OK(hipMemcpyAsync(d_a.p, albedo, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(d_n.p, normal, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (zdepth) HIP_OK(hipMemcpyAsync(d_z.p, zdepth, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return ZR_OK;
}

}  // namespace

// the checks of a zr_denoise_guided_params, which need no device
int check_guided_params(const zr_denoise_guided_params* dp) {
    if (dp->iterations < 0 || dp->iterations > 8) return fail(ZR_E_INVALID, "denoise iterations %d outside 0..8", dp->iterations);
    auto positive = [](float v) { return v > 0.0f && std::isfinite(v); };
    if (!positive(dp->sigma_variance) || !positive(dp->sigma_normal) || !positive(dp->sigma_albedo) || !(dp->sigma_depth >= 0.0f) || !std::isfinite(dp->sigma_depth))
        return fail(ZR_E_INVALID, "denoise sigmas must be positive and finite (sigma_depth: >= 0, 0 = no depth guide)");
    if (!positive(dp->epsilon)) return fail(ZR_E_INVALID, "denoise epsilon %g is not positive and finite", (double)dp->epsilon);
    return ZR_OK;
}

// The guided filter on device frames of n = W * H pixels: d_c / d_v hold colour and variance and receive the results; the guides are uploaded from the host.
int denoise_guided_device(zr_ctx* c, const zr_denoise_guided_params* dp, DevBuf<double>& d_c, DevBuf<double>& d_v, const double* albedo, const double* normal,
                          const double* zdepth, int W, int H, double* out, double* out_variance) {
    const size_t n = (size_t)W * H;
    DevBuf<double> d_a, d_n, d_z; DevBuf<float4> col0, col1, var0, var1, g0, g1;
    int rc;
    if ((rc = upload_guides(c, albedo, normal, zdepth, n, d_a, d_n, d_z))) return rc;
    if ((rc = col0.alloc(n)) || (rc = col1.alloc(n)) || (rc = var0.alloc(n)) || (rc = var1.alloc(n)) || (rc = g0.alloc(n)) || (rc = g1.alloc(n))) return rc;
    // colour and variance have been packed before the unpack kernels overwrite them
    HIP_OK(zr::launch_denoise_guided(d_c.p, d_v.p, d_a.p, d_n.p, zdepth ? d_z.p : nullptr, W, H, *dp, col0.p, col1.p, var0.p, var1.p, g0.p, g1.p, d_c.p,
                                     out_variance ? d_v.p : nullptr, c->stream));
    HIP_OK(hipMemcpyAsync(out, d_c.p, n * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (out_variance) HIP_OK(hipMemcpyAsync(out_variance, d_v.p, n * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return ZR_OK;
}

// the checks of a zr_denoise_nlm_params, which need no device
int check_nlm_params(const zr_denoise_nlm_params* dp) {
    if (dp->search_radius < 0 || dp->search_radius > 10) return fail(ZR_E_INVALID, "denoise search radius %d outside 0..10", dp->search_radius);
    if (dp->patch_radius < 0 || dp->patch_radius > 3) return fail(ZR_E_INVALID, "denoise patch radius %d outside 0..3", dp->patch_radius);
    auto positive = [](float v) { return v > 0.0f && std::isfinite(v); };
    if (!positive(dp->k)) return fail(ZR_E_INVALID, "denoise distance scale k %g is not positive and finite", (double)dp->k);
    if (!(dp->alpha >= 0.0f) || !std::isfinite(dp->alpha)) return fail(ZR_E_INVALID, "denoise variance cancellation alpha %g is negative or not finite", (double)dp->alpha);
    if (!positive(dp->sigma_normal) || !positive(dp->sigma_albedo)) return fail(ZR_E_INVALID, "denoise sigmas must be positive and finite");
    if (!positive(dp->epsilon)) return fail(ZR_E_INVALID, "denoise epsilon %g is not positive and finite", (double)dp->epsilon);
    return ZR_OK;
}

// The non-local-means filter on device frames of n = W * H pixels: d_a / d_b hold the halves and receive out / out_error; the guides are uploaded from the host.
int denoise_nlm_device(zr_ctx* c, const zr_denoise_nlm_params* dp, DevBuf<double>& d_a, DevBuf<double>& d_b, DevBuf<double>& d_v, const double* albedo,
                       const double* normal, int W, int H, double* out, double* out_error) {
    const size_t n = (size_t)W * H;
    DevBuf<double> d_al, d_n, d_z; DevBuf<float4> ua, ub, vh, vs, g0, g1;
    int rc;
    if ((rc = upload_guides(c, albedo, normal, nullptr, n, d_al, d_n, d_z))) return rc;
    if ((rc = ua.alloc(n)) || (rc = ub.alloc(n)) || (rc = vh.alloc(n)) || (rc = vs.alloc(n)) || (rc = g0.alloc(n)) || (rc = g1.alloc(n))) return rc;
    // the halves have been packed before the filter kernel overwrites them
    HIP_OK(zr::launch_denoise_nlm(d_a.p, d_b.p, d_v.p, d_al.p, d_n.p, W, H, *dp, ua.p, ub.p, vh.p, vs.p, g0.p, g1.p, d_a.p, out_error ? d_b.p : nullptr, c->stream));
    HIP_OK(hipMemcpyAsync(out, d_a.p, n * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (out_error) HIP_OK(hipMemcpyAsync(out_error, d_b.p, n * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return ZR_OK;
}

}  // namespace zr_host

extern "C" {

int zr_post_process(zr_ctx* c, const zr_post_params* pp, const double* frame, int W, int H, int is_data_pass, int apply_gamma, uint8_t* out) {
    if (!c || !pp || !frame || !out) return fail(ZR_E_INVALID, "null argument");
    int rc = check_frame_size(W, H, 2);
    if (rc) return rc;
    if (pp->use_bloom && (pp->bloom_radius < 0 || pp->bloom_radius > 4096)) return fail(ZR_E_INVALID, "bloom radius out of range");
    HIP_OK(hipSetDevice(c->device));
    const size_t n = (size_t)W * H;
    DevBuf<double> d_frame, t0, t1, t2; DevBuf<uint8_t> d_out;
    if ((rc = d_frame.alloc(n * 3)) || (rc = d_out.alloc(n * 3))) return rc;
    const bool bloom = !is_data_pass && pp->use_bloom, sharpen = !is_data_pass && pp->use_sharpening;
    if (bloom && ((rc = t0.alloc(n * 3)) || (rc = t1.alloc(n * 3)))) return rc;
    if (sharpen && (rc = t2.alloc(n * 3))) return rc;
    HIP_OK(hipMemcpyAsync(d_frame.p, frame, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const double ev = std::pow(2.0, (double)pp->exposure);   // camera.hpp:711
    HIP_OK(zr::launch_post(d_frame.p, W, H, *pp, is_data_pass, apply_gamma, ev, t0.p, t1.p, t2.p, d_out.p, c->stream));
    HIP_OK(hipMemcpyAsync(out, d_out.p, n * 3, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return ZR_OK;
}

int zr_denoise(zr_ctx* c, const zr_denoise_params* dp, const double* color, const double* albedo, const double* normal, const double* zdepth,
               int W, int H, double* out) {
    if (!c || !dp || !color || !albedo || !normal || !out) return fail(ZR_E_INVALID, "null argument");
    int rc = check_frame_size(W, H, 1);
    if (rc) return rc;
    if (dp->iterations < 0 || dp->iterations > 8) return fail(ZR_E_INVALID, "denoise iterations %d outside 0..8", dp->iterations);
    if (!(dp->sigma_color > 0.0f) || !(dp->sigma_normal > 0.0f) || !(dp->sigma_albedo > 0.0f) || dp->sigma_depth < 0.0f || std::isnan(dp->sigma_depth))
        return fail(ZR_E_INVALID, "denoise sigmas must be positive (sigma_depth: >= 0, 0 = no depth guide)");
    HIP_OK(hipSetDevice(c->device));
    const size_t n = (size_t)W * H;
    DevBuf<double> d_c, d_a, d_n, d_z; DevBuf<float4> col0, col1, g0, g1;
    if ((rc = d_c.alloc(n * 3))) return rc;
    HIP_OK(hipMemcpyAsync(d_c.p, color, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((rc = upload_guides(c, albedo, normal, zdepth, n, d_a, d_n, d_z))) return rc;
    if ((rc = col0.alloc(n)) || (rc = col1.alloc(n)) || (rc = g0.alloc(n)) || (rc = g1.alloc(n))) return rc;
    // the colour frame has been packed before the unpack kernel overwrites it
    HIP_OK(zr::launch_denoise(d_c.p, d_a.p, d_n.p, zdepth ? d_z.p : nullptr, W, H, *dp, col0.p, col1.p, g0.p, g1.p, d_c.p, c->stream));
    HIP_OK(hipMemcpyAsync(out, d_c.p, n * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return ZR_OK;
}

int zr_denoise_guided(zr_ctx* c, const zr_denoise_guided_params* dp, const double* color, const double* variance, const double* albedo, const double* normal,
                      const double* zdepth, int W, int H, double* out, double* out_variance) {
    if (!c || !dp || !color || !variance || !albedo || !normal || !out) return fail(ZR_E_INVALID, "null argument");
    int rc = check_frame_size(W, H, 1);
    if (rc || (rc = check_guided_params(dp))) return rc;
    HIP_OK(hipSetDevice(c->device));
    const size_t n = (size_t)W * H;
    DevBuf<double> d_c, d_v;
    if ((rc = d_c.alloc(n * 3)) || (rc = d_v.alloc(n * 3))) return rc;
    HIP_OK(hipMemcpyAsync(d_c.p, color, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(d_v.p, variance, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return denoise_guided_device(c, dp, d_c, d_v, albedo, normal, zdepth, W, H, out, out_variance);
}

int zr_denoise_nlm(zr_ctx* c, const zr_denoise_nlm_params* dp, const double* half_a, const double* half_b, const double* variance, const double* albedo,
                   const double* normal, int W, int H, double* out, double* out_error) {
    if (!dp) return fail(ZR_E_INVALID, "null argument");
    int rc = check_nlm_params(dp);   // the parameters first: they need no device and no other argument
    if (rc) return rc;
    if (!c || !half_a || !half_b || !variance || !albedo || !normal || !out) return fail(ZR_E_INVALID, "null argument");
    if ((rc = check_frame_size(W, H, 1))) return rc;
    HIP_OK(hipSetDevice(c->device));
    const size_t n = (size_t)W * H;
    DevBuf<double> d_a, d_b, d_v;
    if ((rc = d_a.alloc(n * 3)) || (rc = d_b.alloc(n * 3)) || (rc = d_v.alloc(n * 3))) return rc;
    HIP_OK(hipMemcpyAsync(d_a.p, half_a, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(d_b.p, half_b, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipMemcpyAsync(d_v.p, variance, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return denoise_nlm_device(c, dp, d_a, d_b, d_v, albedo, normal, W, H, out, out_error);
}

int zr_sharpen_frame(zr_ctx* c, const double* in, int W, int H, double amount, double* out) {
    if (!c || !in || !out) return fail(ZR_E_INVALID, "null argument");
    int rc = check_frame_size(W, H, 1);
    if (rc) return rc;
    const size_t n = (size_t)W * H;
    if (!(amount > 0.0)) {   // color_processing.hpp:208-210: nothing to do
        if (out != in) std::memmove(out, in, n * 3 * sizeof(double));
        return ZR_OK;
    }
    HIP_OK(hipSetDevice(c->device));
    DevBuf<double> d_in, d_out;
    if ((rc = d_in.alloc(n * 3)) || (rc = d_out.alloc(n * 3))) return rc;
    HIP_OK(hipMemcpyAsync(d_in.p, in, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_OK(zr::launch_sharpen(d_in.p, d_out.p, W, H, amount, c->stream));
    HIP_OK(hipMemcpyAsync(out, d_out.p, n * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return ZR_OK;
}

int zr_analyze_frame(zr_ctx* c, const double* frame, size_t n, zr_image_stats* out) {
    if (!c || !frame || !out) return fail(ZR_E_INVALID, "null argument");
    if (n == 0 || n > (1ull << 31)) return fail(ZR_E_INVALID, "pixel count not supported");
    HIP_OK(hipSetDevice(c->device));
    const size_t blocks = (n + 255) / 256;
    DevBuf<double> d_frame, d_log; DevBuf<float> d_max; DevBuf<int> d_hist;
    int rc;
    if ((rc = d_frame.alloc(n * 3)) || (rc = d_log.alloc(blocks)) || (rc = d_max.alloc(blocks)) || (rc = d_hist.alloc(256))) return rc;
    HIP_OK(hipMemcpyAsync(d_frame.p, frame, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_OK(zr::launch_analyze(d_frame.p, n, d_log.p, d_max.p, d_hist.p, c->stream));
    std::vector<double> plog(blocks); std::vector<float> pmax(blocks);
    HIP_OK(hipMemcpyAsync(plog.data(), d_log.p, blocks * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(pmax.data(), d_max.p, blocks * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(out->histogram, d_hist.p, 256 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    double total = 0.0; float mx = 0.0f;
    for (size_t b = 0; b < blocks; b++) { total += plog[b]; if (pmax[b] > mx) mx = pmax[b]; }
    out->max_luminance = mx;
    out->average_luminance = std::pow(2.0f, static_cast<float>(total / (double)n));   // color_processing.hpp:180
    return ZR_OK;
}

}  // extern "C"
