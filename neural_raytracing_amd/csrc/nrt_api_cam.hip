// nrt_api_cam.hip -- ray generation, frames and composite launchers
#include "nrt_launch.h"

using namespace nrt;

extern "C" {
int nrt_raygen(const nrt_camera* cams, int32_t N, int32_t x0, int32_t y0, int32_t W, int32_t H,
               float with_noise, const float* noise, const float* positions, float* rays,
               void* stream) {
  if (!cams || N < 1 || W < 0 || H < 0 || !rays) { set_error("nrt_raygen: bad argument"); return NRT_EINVAL; }
  const int64_t total = (int64_t)N * W * H;
  if (total == 0) return NRT_OK;
  hipStream_t st = (hipStream_t)stream;
  nrt_camera* dcam = nullptr;
  NRT_HIP(hipMallocAsync((void**)&dcam, sizeof(nrt_camera) * N, st));
  NRT_HIP(hipMemcpyAsync(dcam, cams, sizeof(nrt_camera) * N, hipMemcpyHostToDevice, st));
  k_raygen<><<<dim3(ceil_div64(total, 256)), dim3(256), 0, st>>>(dcam, N, x0, y0, W, H, with_noise, noise, positions, rays);
  int rc = check_launch("k_raygen");
  (void)hipFreeAsync(dcam, st);
  return rc;
}

static bool mm_bad(const float* t, const float* angle, const float* axis, const float* focals,
                   int32_t N, int32_t size, int32_t W, int32_t H) {
  return !t || !angle || !axis || !focals || N < 1 || N > 65535 || size < 1 || W < 0 || H < 0;
}
static int64_t mm_blocks(int64_t m) { return std::max<int64_t>(1, (m + kMMSlice - 1) / kMMSlice); }

int nrt_raygen_mm(const float* t, const float* angle, const float* axis, const float* focals,
                  int32_t N, int32_t size, int32_t x0, int32_t y0, int32_t W, int32_t H,
                  float with_noise, const float* noise, const float* positions, float* rays,
                  void* stream) {
  if (mm_bad(t, angle, axis, focals, N, size, W, H) || !rays) {
    set_error("nrt_raygen_mm: bad argument");
    return NRT_EINVAL;
  }
  const int64_t total = (int64_t)N * W * H;
  if (total == 0) return NRT_OK;
  k_raygen_mm<><<<dim3(ceil_div64(total, 256)), dim3(256), 0, (hipStream_t)stream>>>(
      t, angle, axis, focals, N, size, x0, y0, W, H, with_noise, noise, positions, rays);
  return check_launch("k_raygen_mm");
}

size_t nrt_raygen_mm_backward_workspace_bytes(int32_t N, int32_t W, int32_t H) {
  const int64_t m = (int64_t)std::max(W, 0) * std::max(H, 0);
  return (size_t)std::max(N, 1) * (size_t)mm_blocks(m) * kMMCols * sizeof(float);
}

int nrt_raygen_mm_backward(const float* t, const float* angle, const float* axis,
                           const float* focals, int32_t N, int32_t size, int32_t x0, int32_t y0,
                           int32_t W, int32_t H, float with_noise, const float* noise,
                           const float* positions, const float* d_rays, float* d_t,
                           float* d_angle, float* d_axis, float* d_focals, void* workspace,
                           void* stream) {
  if (mm_bad(t, angle, axis, focals, N, size, W, H) || !workspace ||
      (!d_rays && (int64_t)W * H > 0)) {
    set_error("nrt_raygen_mm_backward: bad argument");
    return NRT_EINVAL;
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t nb = mm_blocks((int64_t)W * H);
  if (nb > 0x7fffffff) { set_error("nrt_raygen_mm_backward: tile too large"); return NRT_EUNSUPPORTED; }
  float* partial = (float*)workspace;
  k_raygen_mm_bwd_partial<><<<dim3((unsigned)nb, (unsigned)N), dim3(kMMThreads), 0, st>>>(
      angle, axis, focals, size, x0, y0, W, H, with_noise, noise, positions, d_rays, partial);
  if (int rc = check_launch("k_raygen_mm_bwd_partial")) return rc;
  k_raygen_mm_bwd_final<><<<dim3(ceil_div64((int64_t)N * kMMCols, 256)), dim3(256), 0, st>>>(
      partial, (int)nb, N, d_t, d_angle, d_axis, d_focals);
  return check_launch("k_raygen_mm_bwd_final");
}

int nrt_composite(const float* rgb, const float* thr, const uint8_t* hit, int32_t N, int32_t W,
                  int32_t H, int32_t alpha, int32_t fill, float bg, float* img, int32_t IW,
                  int32_t IH, int32_t C, int32_t X0, int32_t Y0, void* stream) {
  if (!rgb || !img || (alpha && !thr) || (fill && !hit)) { set_error("nrt_composite: bad argument"); return NRT_EINVAL; }
  const int64_t total = (int64_t)N * W * H;
  if (total == 0) return NRT_OK;
  if (X0 < 0 || Y0 < 0 || X0 + W > IW || Y0 + H > IH) { set_error("nrt_composite: tile outside image"); return NRT_EINVAL; }
  k_composite<><<<dim3(ceil_div64(total, 256)), dim3(256), 0, (hipStream_t)stream>>>(
      rgb, thr, hit, N, W, H, alpha, fill, bg, img, IW, IH, C, X0, Y0);
  return check_launch("k_composite");
}


}  // extern "C"
