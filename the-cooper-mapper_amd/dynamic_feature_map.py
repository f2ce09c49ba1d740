"""Host-side mirror of ``lidar_slam::DynamicFeatureMap`` (util/DynamicFeatureMap.h) on the paged mode
of the device-resident localisation node (``lslam_pmap_open``, ``csrc/lslam_loc.hip``): a window of W x H x D cubes
addressed by global cube index follows the sensor; ``update`` reads, filters and gives a kd-tree to exactly the cubes that
enter the window, ``scan_match_scan`` is ``FeatureMap::scanMatchScan``'s arithmetic over the window.

``addFeatureCloud`` / ``downsizeValidCloud`` (LaserMatcher.cpp:350 never adds in dynamic mode), ``saveCloudToFiles`` (its body
is commented out) and ``getFullMap`` (gated on cubes nothing fills) are not mirrored.
"""
import ctypes as C

import numpy as np

from .capi import LslamError, load_library
from .laser_localization import LaserLocalization


def convert_index_file(in_path, x, y, z, out_path):
    """convertIndexFile: ``count type i-x j-y k-z size`` for every line of an index.txt, each line once.  No device needed."""
    lib = load_library()
    rc = lib.lslam_index_convert(str(in_path).encode(), int(x), int(y), int(z), str(out_path).encode())
    if rc < 0:
        raise LslamError(rc, lib.lslam_last_error().decode())


class DynamicFeatureMap:
    """Defaults of DynamicFeatureMap.h:76-90: 21 x 11 x 21 cubes of 50 m, valid distance 100 m, leaves 0.2 / 0.4 / 0.6."""

    def __init__(self, ctx, cube_width=21, cube_height=11, cube_depth=21):
        self.ctx = ctx
        self._node = LaserLocalization(ctx, cube_width, cube_height, cube_depth, map_filter_corner=0.2, map_filter_surf=0.4,
                                       cube_size=50.0, lidar_valid_distance=100.0)
        self._opened = False

    def close(self):
        self._node.close()

    def _closed_only(self, what):
        if self._opened:
            raise ValueError(what + " must be set before setup_files_directory")

    def setup_filter_size(self, corner, surf, map=0.6):
        """The leaves the entering cubes are filtered with (the third is getFullMap's, which is not built)."""
        self._closed_only("filter sizes")
        n = self._node
        n._check(n.lib.lslam_loc_setup_map_filter_size(n.h, float(corner), float(surf)))

    def setup_world_cube_size(self, size):
        self._closed_only("the cube size")
        n = self._node
        n._check(n.lib.lslam_loc_setup_world_cube_size(n.h, float(size)))

    def setup_lidar_valid_distance(self, dist):
        n = self._node
        n._check(n.lib.lslam_loc_setup_lidar_valid_distance(n.h, float(dist)))

    def setup_lidar_fov(self, max_up_deg, max_down_deg):
        """Accepted and ignored: InVerticalFov computes the angles and decides by distance alone."""

    def setup_scan_filter_size(self, corner, surf):
        n = self._node
        n._check(n.lib.lslam_loc_setup_scan_filter_size(n.h, float(corner), float(surf)))

    def setup_paged_capacity(self, max_points_per_type):
        self._node.setup_paged_capacity(max_points_per_type)

    def setup_files_directory(self, directory):
        self._node.setup_files_directory(directory)
        self._opened = True

    convert_index_file = staticmethod(convert_index_file)

    def update(self, sensor_position, sensor_up_dir=None):
        """update(sensorGlo, sensorUpDir); the up direction decides nothing in the reference and is ignored."""
        self._node.update(sensor_position)

    def stage(self, position):
        self._node.stage(position)

    def get_surround_feature(self):
        return self._node.get_window_surround()

    def scan_match_scan(self, corner, surf, pose):
        """scanMatchScan(corner, surf, transformf) after an update at the Twist's translation -> (ok, pose, stats).  The clouds go
        through the node's scan filters first (lslam_loc_match is prepareFeatureFrame + optimizeTransform; leaves 1.0 / 1.0 unless
        setup_scan_filter_size says otherwise)."""
        status, p, st = self._node.match(corner, surf, pose)
        return status == 0, p, st

    def window_info(self):
        return self._node.window_info()
