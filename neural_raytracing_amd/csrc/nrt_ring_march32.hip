// FP32 (reference-precision) march + coarse scan on the block-cooperative LDS weight ring
// (k_march32 / k_scan_best32, nrt_device.h ring32): same job lists and persistent grid as the
// FP16 ring march (nrt_ring_march.hip), 16-ray tiles; accurate sincosf / sqrtf / expf and
// softplus_exact (a few ulp of torch's log1pf(expf), nrt_device.h).
#include "nrt_launch.h"

// waves per block of the 128-wide SDFs' FP32 ring march (timing experiments: -DNRT_R32_SMALL_WV)
#ifndef NRT_R32_SMALL_WV
#define NRT_R32_SMALL_WV 8
#endif

namespace nrt {

int ring32_launch(const nrt_sdf* s, Pass pass, const float* rays, int64_t P, const MarchArgs& ma,
                  const MarchOut& out, hipStream_t st) {
  return ring32_dispatch(s, [&]<int KH, int KE, int ACT>() -> int {
    constexpr int WV = KH <= 32 ? NRT_R32_SMALL_WV : kRing32Waves;
    const size_t lds = ring32::Engine<KH, KE, WV>::lds_bytes(s->mlp->host_dev.freqs, ring_bias_bytes(s),
                                                             ring32_sphere_bytes(s));
    auto launch = [&](auto kern, const char* name, MarchLaunch how = {}) -> int {
      return launch_march(kern, name, 64 * WV, lds, s, rays, P, ma, out, how, st);
    };
    switch (pass) {
      case Pass::March: return launch(k_march32<KH, KE, WV, ACT>, "k_march32", {.stage_lines = true});
      case Pass::ScanBest: return launch(k_scan_best32<KH, KE, WV, ACT>, "k_scan_best32");
      case Pass::Occlusion: return launch(k_occl32<KH, KE, WV, ACT>, "k_occl32");
      default: set_error("FP32 ring engine: no such pass"); return NRT_EINVAL;
    }
  });
}

int ring_march32(const nrt_sdf* s, const float* rays, int64_t P, const MarchArgs& ma, float* t,
                 uint8_t* hit, float* p, float* n, float* raw_n, float* thr, int32_t* idx,
                 int32_t* cnt, unsigned long long* keys, hipStream_t st) {
  const MarchOut out{.t = t, .thr = thr, .keys = keys};
  if (ma.primary) NRT_HIP(hipMemsetAsync(keys, 0xff, (size_t)P * sizeof(unsigned long long), st));
  if (int rc = ring32_launch(s, Pass::March, rays, P, ma, out, st)) return rc;
  if (ma.primary)
    if (int rc = ring32_launch(s, Pass::ScanBest, rays, P, ma, out, st)) return rc;
  return march_finish(rays, P, t, hit, p, n, raw_n, idx, cnt, st);
}

}  // namespace nrt
