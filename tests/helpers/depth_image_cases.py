"""The views and settings shared by the CPU and the GPU tests of the depth image path, so that what the CPU test asserts
about a case (its band placement) is asserted about the very case the GPU test runs."""
import functools

import numpy as np

import depth_feed_ref as R
import depth_image_ref as I
from dddmr_navigation_amd import scenes

TBS_CAM = (0.2, 0.0, 0.3) + tuple(scenes.quat_from_rpy(0.0, 0.05, 0.0))      # camera_link on the robot, slightly nose-down
TBO_CAM = R.compose(TBS_CAM, scenes.T_LINK_OPTICAL)                          # base <- optical
POSES = [(0.0, 0.0, 0.0) + tuple(scenes.quat_from_rpy(0.0, 0.0, 0.0)),
         (-1.0, 0.2, 0.0) + tuple(scenes.quat_from_rpy(0.0, 0.02, 0.3))]
SHIPPED = dict(max_distance=6.0, leaf_size=0.05, sample_step=4)              # multi_depth_camera_3d_ros_launch.py
DEFAULTS = dict(max_distance=4.0, leaf_size=0.05, sample_step=2)            # the node's declare_parameter defaults
MIN_GAP = 2e-4


@functools.lru_cache(maxsize=None)
def _cloud():
    return scenes.cloud_c2()


@functools.lru_cache(maxsize=32)
def render(width, height, pose, seed, tbs=TBS_CAM):
    """-> (uint16 image, (fx, fy, cx, cy)) of the C2 scene from POSES[pose] (or a pose tuple)"""
    tgb = POSES[pose] if isinstance(pose, int) else pose
    return scenes.depth_image(_cloud(), R.compose(tgb, tbs), width, height, 1.5, 1.0, 8.0, seed=seed)


def end_to_end_cases():
    """(name, pose index, seed, node settings): 848 x 480 at the shipped settings and at the defaults, two poses"""
    return [("shipped-pose0", 0, 21, SHIPPED), ("shipped-pose1", 1, 22, SHIPPED),
            ("defaults-pose0", 0, 23, DEFAULTS), ("defaults-pose1", 1, 24, DEFAULTS)]


def end_to_end_band(pose, seed, node):
    img, K4 = render(848, 480, pose, seed)
    return I.decided_band(img, K4, TBO_CAM, node)
