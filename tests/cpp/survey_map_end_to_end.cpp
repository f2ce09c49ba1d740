// C++ drop-in check of include/lslam_survey_map.hpp: the featureExtracter workflow through the mirrors.  argv: a file of packed
// {x, y, z} floats (the survey cloud), a directory to save into, the partition leaf.  extract -> saveCloudToFiles ->
// LaserLocalization::loadMap of that directory; "OK extract <corner> <surf> <blocks kept> <blocks dropped>" and
// "OK loaded <corner points> <surf points>" for the test to compare.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lslam_pipeline.hpp"
#include "lslam_scan_match.hpp"
#include "lslam_survey_map.hpp"

struct Xyz {
  float x, y, z;
};

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  lidar_slam::ScanMatch sm(10);  // owns the context; never throws
  if (!sm.ok()) {
    std::fprintf(stderr, "backend unavailable: %s\n", sm.initError().c_str());
    return 1;
  }
  std::vector<Xyz> cloud;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  Xyz p;
  while (std::fread(&p, sizeof(p), 1, f) == 1) cloud.push_back(p);
  std::fclose(f);
  lidar_slam::FeatureExtracter fx(sm.context());
  fx.params().partition_leaf = (float)std::atof(argv[3]);
  lslam_survey_stats st;
  if (!fx.ok() || !fx.extract(cloud) || !fx.stats(&st) || !fx.saveCloudToFiles(argv[2])) {
    std::fprintf(stderr, "extraction failed: %s\n", fx.lastError().c_str());
    return 1;
  }
  std::vector<float> corner, surf;
  if (!fx.getFeatureClouds(corner, surf) || corner.size() != (size_t)st.n_corner * 4 || surf.size() != (size_t)st.n_surf * 4) return 1;
  std::printf("OK extract %lld %lld %lld %lld\n", (long long)st.n_corner, (long long)st.n_surf, (long long)st.blocks_kept,
              (long long)st.blocks_dropped);
  const lslam_survey_params &P = fx.params();
  lidar_slam::LaserLocalization localization(sm.context(), P.cube_dims[0], P.cube_dims[1], P.cube_dims[2]);
  if (!localization.ok() || !localization.setupWorldOrigin(P.cube_origin[0], P.cube_origin[1], P.cube_origin[2]) ||
      !localization.setupWorldCubeSize(P.cube_size) || !localization.loadMap(argv[2])) {
    std::fprintf(stderr, "map not loaded: %s\n", localization.lastError().c_str());
    return 1;
  }
  lslam_loc_map_stats info;
  if (lslam_loc_info(localization.handle(), &info) != LSLAM_OK) return 1;
  std::printf("OK loaded %llu %llu\n", (unsigned long long)info.n_points[0], (unsigned long long)info.n_points[1]);
  return 0;
}
