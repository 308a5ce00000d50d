// zr_image.cpp — the image-space entry points of the C ABI (include/zr_capi.h), which need a context and no scene: the post stack, the two a-trous denoisers
// (the variance-guided one, also behind zr_accum_denoise), the non-local-means denoiser (also behind zr_accum_denoise_nlm), sharpening and the frame analysis.
#include "zr_frame.h"

namespace zr_host {
namespace {

// a frame an image entry accepts: sides of at least min_side, at most 2^31 pixels
int check_frame_size(int W, int H, int min_side) {
    return W < min_side || H < min_side || (size_t)W * H > (1ull << 31) ? fail(ZR_E_INVALID, "frame size %d x %d not supported", W, H) : ZR_OK;
}

bool positive(float v) { return v > 0.0f && std::isfinite(v); }   // what the guided and the non-local-means parameters ask of a sigma, k or epsilon

// Frame I/O of the image entries: frames of n pixels with three doubles each, in c->stream's order.  upload_frames allocates every d and copies its host frame
// into it; download_frames copies the device frames out, then synchronises the stream.  An entry whose host pointer is null is skipped (an optional guide or
// output): its d stays empty, d->p null.
struct HostFrame { DevBuf<double>* d; const double* host; };
struct DeviceFrame { double* host; const double* d; };
int upload_frames(zr_ctx* c, size_t n, std::initializer_list<HostFrame> frames) {
    for (const HostFrame& f : frames) {
        if (!f.host) continue;
        if (int rc = f.d->alloc(n * 3)) return rc;
        HIP_OK(hipMemcpyAsync(f.d->p, f.host, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    return ZR_OK;
}
int download_frames(zr_ctx* c, size_t n, std::initializer_list<DeviceFrame> frames) {
    for (const DeviceFrame& f : frames)
        if (f.host) HIP_OK(hipMemcpyAsync(f.host, f.d, n * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return ZR_OK;
}

// m float4 scratch planes of n pixels
int alloc_planes(size_t n, std::initializer_list<DevBuf<float4>*> planes) {
    for (DevBuf<float4>* p : planes) if (int rc = p->alloc(n)) return rc;
    return ZR_OK;
}

// The plain a-trous filter on a device frame of n = W * H pixels: d_c holds the colour and receives the result; the guides are uploaded from the host.
int denoise_device(zr_ctx* c, const zr_denoise_params* dp, DevBuf<double>& d_c, const double* albedo, const double* normal, const double* zdepth, int W, int H,
                   double* out) {
    const size_t n = (size_t)W * H;
    DevBuf<double> d_a, d_n, d_z; DevBuf<float4> col0, col1, g0, g1;
    int rc;
    if ((rc = upload_frames(c, n, {{&d_a, albedo}, {&d_n, normal}, {&d_z, zdepth}})) || (rc = alloc_planes(n, {&col0, &col1, &g0, &g1}))) return rc;
    // the colour frame has been packed before the unpack kernel overwrites it
    HIP_OK(zr::launch_denoise(d_c.p, d_a.p, d_n.p, d_z.p, W, H, *dp, col0.p, col1.p, g0.p, g1.p, d_c.p, c->stream));
    return download_frames(c, n, {{out, d_c.p}});
}

}  // namespace

// the checks of a zr_denoise_guided_params, which need no device
int check_guided_params(const zr_denoise_guided_params* dp) {
    if (dp->iterations < 0 || dp->iterations > 8) return fail(ZR_E_INVALID, "denoise iterations %d outside 0..8", dp->iterations);
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
    if ((rc = upload_frames(c, n, {{&d_a, albedo}, {&d_n, normal}, {&d_z, zdepth}})) || (rc = alloc_planes(n, {&col0, &col1, &var0, &var1, &g0, &g1}))) return rc;
    // colour and variance have been packed before the unpack kernels overwrite them
    HIP_OK(zr::launch_denoise_guided(d_c.p, d_v.p, d_a.p, d_n.p, d_z.p, W, H, *dp, col0.p, col1.p, var0.p, var1.p, g0.p, g1.p, d_c.p,
                                     out_variance ? d_v.p : nullptr, c->stream));
    return download_frames(c, n, {{out, d_c.p}, {out_variance, d_v.p}});
}

// the checks of a zr_denoise_nlm_params, which need no device
int check_nlm_params(const zr_denoise_nlm_params* dp) {
    if (dp->search_radius < 0 || dp->search_radius > 10) return fail(ZR_E_INVALID, "denoise search radius %d outside 0..10", dp->search_radius);
    if (dp->patch_radius < 0 || dp->patch_radius > 3) return fail(ZR_E_INVALID, "denoise patch radius %d outside 0..3", dp->patch_radius);
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
    DevBuf<double> d_al, d_n; DevBuf<float4> ua, ub, vh, vs, g0, g1;
    int rc;
    if ((rc = upload_frames(c, n, {{&d_al, albedo}, {&d_n, normal}})) || (rc = alloc_planes(n, {&ua, &ub, &vh, &vs, &g0, &g1}))) return rc;
    // the halves have been packed before the filter kernel overwrites them
    HIP_OK(zr::launch_denoise_nlm(d_a.p, d_b.p, d_v.p, d_al.p, d_n.p, W, H, *dp, ua.p, ub.p, vh.p, vs.p, g0.p, g1.p, d_a.p, out_error ? d_b.p : nullptr, c->stream));
    return download_frames(c, n, {{out, d_a.p}, {out_error, d_b.p}});
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
    if ((rc = upload_frames(c, n, {{&d_frame, frame}})) || (rc = d_out.alloc(n * 3))) return rc;
    const bool bloom = !is_data_pass && pp->use_bloom, sharpen = !is_data_pass && pp->use_sharpening;
    if (bloom && ((rc = t0.alloc(n * 3)) || (rc = t1.alloc(n * 3)))) return rc;
    if (sharpen && (rc = t2.alloc(n * 3))) return rc;
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
    DevBuf<double> d_c;
    if ((rc = upload_frames(c, (size_t)W * H, {{&d_c, color}}))) return rc;
    return denoise_device(c, dp, d_c, albedo, normal, zdepth, W, H, out);
}

int zr_denoise_guided(zr_ctx* c, const zr_denoise_guided_params* dp, const double* color, const double* variance, const double* albedo, const double* normal,
                      const double* zdepth, int W, int H, double* out, double* out_variance) {
    if (!c || !dp || !color || !variance || !albedo || !normal || !out) return fail(ZR_E_INVALID, "null argument");
    int rc = check_frame_size(W, H, 1);
    if (rc || (rc = check_guided_params(dp))) return rc;
    HIP_OK(hipSetDevice(c->device));
    DevBuf<double> d_c, d_v;
    if ((rc = upload_frames(c, (size_t)W * H, {{&d_c, color}, {&d_v, variance}}))) return rc;
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
    DevBuf<double> d_a, d_b, d_v;
    if ((rc = upload_frames(c, (size_t)W * H, {{&d_a, half_a}, {&d_b, half_b}, {&d_v, variance}}))) return rc;
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
    if ((rc = upload_frames(c, n, {{&d_in, in}})) || (rc = d_out.alloc(n * 3))) return rc;
    HIP_OK(zr::launch_sharpen(d_in.p, d_out.p, W, H, amount, c->stream));
    return download_frames(c, n, {{out, d_out.p}});
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
