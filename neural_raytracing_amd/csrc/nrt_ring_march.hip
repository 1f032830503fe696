// FP16 march + coarse scan on the block-cooperative LDS weight ring (k_march16), load-balanced
// job lists on a persistent grid; then sdf(best) (mode 1) and the hit list.
#include "nrt_launch.h"

namespace nrt {

int ring16_launch(const nrt_sdf* s, Pass pass, const float* rays, int64_t P, const MarchArgs& ma,
                  const MarchOut& out, hipStream_t st) {
  const size_t bias_bytes = ring_bias_bytes(s);
  return ring_dispatch(s, [&]<int NB, int NE, bool FOLD>() -> int {
    // the SphereSDF table goes into LDS behind the ring when it fits and costs no resident block
    // (spheres_value_halves: the two lanes of a ray split the spheres; colocate's 64 spheres:
    // k_march16 51.3 -> 43.8 ms); a table of a few spheres stays on scalar loads
    constexpr int kLdsSpheresMin = 8;
    const size_t base = ring::Cfg<NB, NE, kRingWaves>::lds_bytes(bias_bytes);
    const size_t ring_lds = (base + 15) & ~size_t(15);
    const size_t sph = s->host_dev.kind == 2
                           ? (size_t)ring::sphere_pair_records(s->host_dev.n_spheres) * ring::kSpherePairF4 * 16
                           : 0;  // the pair table (ring::build_sphere_pairs)
    MarchArgs a = ma;
    a.lds_spheres = (sph > 0 && s->host_dev.n_spheres >= kLdsSpheresMin && ring_lds + sph <= (size_t)kLdsBytes &&
                     kLdsBytes / (ring_lds + sph) == kLdsBytes / base) ? (int)ring_lds : 0;
    const size_t lds = a.lds_spheres ? ring_lds + sph : base;
    auto launch = [&](auto kern, const char* name, MarchLaunch how = {}) -> int {
      return launch_march(kern, name, 64 * kRingWaves, lds, s, rays, P, a, out, how, st);
    };
    // the shadow march and NRT_MIXED's flagging march are their own instantiations (the plain
    // march carries none of them); only the plain march stages its lines
    switch (pass) {
      case Pass::March:
        return launch(k_march16<NB, NE, kRingWaves, FOLD>, "k_march16",
                      {.stage_lines = true, .keep_blocks_per_cu = true});
      case Pass::RefineMarch: return launch(k_march16<NB, NE, kRingWaves, FOLD, true>, "k_march16");
      case Pass::ScanBest: return launch(k_scan_best16<NB, NE, kRingWaves, FOLD>, "k_scan_best16");
      case Pass::Occlusion: return launch(k_occl16<NB, NE, kRingWaves, FOLD>, "k_occl16");
      default: set_error("ring engine: no such pass"); return NRT_EINVAL;
    }
  });
}

int ring_march(const nrt_sdf* s, const float* rays, int64_t P, const MarchArgs& ma, float* t,
               uint8_t* hit, float* p, float* n, float* raw_n, float* thr, int32_t* idx,
               int32_t* cnt, unsigned long long* keys, hipStream_t st) {
  const bool scan = ma.primary != 0;
  const MarchOut out{.t = t, .thr = thr, .keys = keys};
  if (scan) NRT_HIP(hipMemsetAsync(keys, 0xff, (size_t)P * sizeof(unsigned long long), st));
  if (int rc = ring16_launch(s, Pass::March, rays, P, ma, out, st)) return rc;
  // option "scan_best32": sdf(best) on the FP32 engine -- the throughput -1000 sdf(best)
  // (sdfs.py:137) multiplies the FP16 SDF error by 1000 in the alpha logit
  if (scan) {
    const bool best32 = option(OPT_SCAN_BEST32) != 0 && ring32_supported(s);
    if (int rc = best32 ? ring32_launch(s, Pass::ScanBest, rays, P, ma, out, st)
                        : ring16_launch(s, Pass::ScanBest, rays, P, ma, out, st))
      return rc;
  }
  return march_finish(rays, P, t, hit, p, n, raw_n, idx, cnt, st);
}

}  // namespace nrt
