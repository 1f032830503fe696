// fp32-split march + coarse scan (k_march3 / k_scan_best3, nrt_ring3.h): the FP32 ring's job
// lists, persistent grid and 16-ray tiles, with every SDF MLP layer on FP16 MFMA at FP32 accuracy
// (hi/lo operand halves, three products per block).
#include "nrt_launch.h"

namespace nrt {

int ring3_launch(const nrt_sdf* s, Pass pass, const float* rays, int64_t P, const MarchArgs& ma,
                 const MarchOut& out, hipStream_t st) {
  return ring3_dispatch(s, [&]<int KH, int KQ, int ACT>() -> int {
    constexpr int WV = kRing3Waves;
    const size_t lds = ring3::Engine<KH, KQ, WV>::lds_bytes(s->mlp->host_dev.freqs, ring_bias_bytes(s),
                                                            ring32_sphere_bytes(s));
    auto launch = [&](auto kern, const char* name, MarchLaunch how = {}) -> int {
      return launch_march(kern, name, 64 * WV, lds, s, rays, P, ma, out, how, st);
    };
    // (profile names: NRT_MIXED's refinement launches apart from the plain ones)
    switch (pass) {
      case Pass::March: return launch(k_march3<KH, KQ, WV, ACT>, "k_march3", {.stage_lines = true});
      case Pass::ScanBest: return launch(k_scan_best3<KH, KQ, WV, ACT>, "k_scan_best3");
      case Pass::Occlusion: return launch(k_occl3<KH, KQ, WV, ACT>, "k_occl3");
      case Pass::RefineMarch: return launch(k_march3<KH, KQ, WV, ACT, true>, "k_refine3");
      case Pass::RefineScan: return launch(k_scan_best3<KH, KQ, WV, ACT, true>, "k_best3");
      case Pass::Eval:  // sdf(p) of [P, 3] points (march_body mode 2)
        return launch(k_sdf_eval3<KH, KQ, WV, ACT>, "k_sdf_eval3", {.schedule_options = false});
    }
    return NRT_EINVAL;
  });
}

int ring_march3(const nrt_sdf* s, const float* rays, int64_t P, const MarchArgs& ma, float* t,
                uint8_t* hit, float* p, float* n, float* raw_n, float* thr, int32_t* idx,
                int32_t* cnt, unsigned long long* keys, hipStream_t st) {
  const MarchOut out{.t = t, .thr = thr, .keys = keys};
  if (ma.primary) NRT_HIP(hipMemsetAsync(keys, 0xff, (size_t)P * sizeof(unsigned long long), st));
  if (int rc = ring3_launch(s, Pass::March, rays, P, ma, out, st)) return rc;
  if (ma.primary)
    if (int rc = ring3_launch(s, Pass::ScanBest, rays, P, ma, out, st)) return rc;
  return march_finish(rays, P, t, hit, p, n, raw_n, idx, cnt, st);
}

}  // namespace nrt
