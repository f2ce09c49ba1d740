// C++ drop-in check of the appearance additions of include/lslam_loop_closure.hpp: KeyframeStore::sc_*,
// LoopDetector::appearance_candidates / detect_appearance over the C ABI.  Reads keyframes written by the test (16 doubles estimate,
// 1 double accumulated distance, then corner and surf clouds as uint32 count + count x {x,y,z,intensity} floats); the last one is
// the new keyframe.  argv[2]: up_axis.  Prints what the test compares with the Python mirror on the same keyframes:
//   NEAREST <loops detect_nearest found>
//   CAND <id> <shift> <distance bits, hex>     one line per listed candidate, best first
//   LOOP <key1 store id> <16 floats>           the accepted loop's relative pose (absent when there is none)
//   SC <keyframes described> <describe launches> <query launches>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <vector>

#include "lslam_loop_closure.hpp"

static bool read_cloud(FILE *f, std::vector<float> &c) {
  uint32_t n = 0;
  if (std::fread(&n, 4, 1, f) != 1) return false;
  c.resize(4 * (size_t)n);
  return n == 0 || std::fread(c.data(), 16, n, f) == n;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  lslam_ctx *ctx = nullptr;
  if (lslam_ctx_create(0, &ctx) != LSLAM_OK) {
    std::fprintf(stderr, "backend unavailable: %s\n", lslam_last_error());
    return 1;
  }
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int rc = 0;
  {
    pose_graph::KeyframeStore store(ctx);
    lslam_sc_params p;
    lslam_sc_default_params(&p);
    p.up_axis = std::atoi(argv[2]);
    if (!store.ok() || !store.sc_setup(&p)) {
      std::fprintf(stderr, "no keyframe store: %s\n", store.lastError().c_str());
      return 1;
    }
    std::vector<pose_graph::KeyFrame::Ptr> all;
    pose_graph::Mat4d est;
    double accum = 0.0;
    std::vector<float> corner, surf;
    while (std::fread(est.m, sizeof(double), 16, f) == 16 && std::fread(&accum, sizeof(double), 1, f) == 1 && read_cloud(f, corner) &&
           read_cloud(f, surf)) {
      pose_graph::KeyFrame::Ptr kf = std::make_shared<pose_graph::KeyFrame>();
      kf->estimate = est;
      kf->accum_distance = accum;
      kf->store_id = store.add(corner, surf);
      kf->store = store.handle();
      if (kf->store_id < 0) {
        std::fprintf(stderr, "add failed: %s\n", store.lastError().c_str());
        return 1;
      }
      all.push_back(kf);
    }
    std::fclose(f);
    if (all.size() < 2) return 2;
    pose_graph::KeyFrame::Ptr nk = all.back();
    all.pop_back();
    pose_graph::LoopDetector det(ctx);
    std::deque<pose_graph::KeyFrame::Ptr> fresh(1, nk);
    std::vector<pose_graph::Loop::Ptr> loops;
    det.detect_nearest(all, fresh, loops);
    std::printf("NEAREST %zu\n", loops.size());
    loops.clear();
    std::vector<int32_t> ids, shifts;
    std::vector<float> dists;
    if (!det.appearance_candidates(all, nk, ids, shifts, dists)) {
      std::fprintf(stderr, "appearance_candidates failed: %s\n", det.lastError().c_str());
      rc = 1;
    }
    for (size_t i = 0; i < ids.size(); ++i) {
      uint32_t bits = 0;
      std::memcpy(&bits, &dists[i], 4);
      std::printf("CAND %d %d %08x\n", (int)ids[i], (int)shifts[i], (unsigned)bits);
    }
    det.detect_appearance(all, fresh, loops);
    for (const auto &lp : loops) {
      std::printf("LOOP %d", lp->key1->store_id);
      for (int i = 0; i < 16; ++i) std::printf(" %.9g", lp->relative_pose.m[i]);
      std::printf("\n");
    }
    lslam_sc_stats st;
    if (!store.sc_info(st)) rc = 1;
    std::printf("SC %lld %lld %lld\n", (long long)st.n_described, (long long)st.describe_launches, (long long)st.query_launches);
  }
  lslam_ctx_destroy(ctx);
  return rc;
}
