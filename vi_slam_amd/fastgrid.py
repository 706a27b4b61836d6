"""Host-side mirror of the grid FAST detector behind vi_slam::geometry::FAST::detect (src/geometry/fast_cuda.cpp:70-132):
vilib::FASTGPU (thirdparty/vilib/visual_lib/include/vilib/feature_detection/fast/fast_gpu.h:44-61) over the C ABI of
include/vslam_fastgrid.h.  Same constructor arguments, same feature grid."""
import ctypes as C

import numpy as np

from ._griddet import GridDetector

SUM_OF_ABS_DIFF_ALL, SUM_OF_ABS_DIFF_ON_ARC, MAX_THRESHOLD = 0, 1, 2  # vilib::fast_score


class _FgParams(C.Structure):  # vslam_fg_params
    _fields_ = [("image_width", C.c_int32), ("image_height", C.c_int32), ("cell_size_width", C.c_int32),
                ("cell_size_height", C.c_int32), ("min_level", C.c_int32), ("max_level", C.c_int32),
                ("horizontal_border", C.c_int32), ("vertical_border", C.c_int32), ("threshold", C.c_float),
                ("min_arc_length", C.c_int32), ("score", C.c_int32), ("tie_rule", C.c_int32), ("device", C.c_int32),
                ("max_batch", C.c_int32)]


class FASTGPU(GridDetector):
    """vilib::FASTGPU(image_width, image_height, cell_size_width, cell_size_height, min_level, max_level,
    horizontal_border, vertical_border, threshold, min_arc_length, score) (fast_gpu.cpp:52-92)."""
    _prefix = "fg"

    def __init__(self, image_width, image_height, cell_size_width=32, cell_size_height=32, min_level=0, max_level=1,
                 horizontal_border=0, vertical_border=0, threshold=10.0, min_arc_length=10, score=SUM_OF_ABS_DIFF_ON_ARC,
                 tie_rule=0, device=0, max_batch=1):
        self._create(_FgParams(image_width, image_height, cell_size_width, cell_size_height, min_level, max_level,
                               horizontal_border, vertical_border, threshold, min_arc_length, score, tie_rule, device, max_batch),
                     min_level, max_level)

    def detect(self, image):
        """Frame(image) + FASTGPU::detect + copyGridToHost -> (pos[cells, 2], score[cells], level[cells])."""
        return self._detect(image)

    def detect_batch(self, images=None, dev_ptrs=None, pitch=None):
        """Several images per pass: host arrays, or device addresses (dev_ptrs, pitch)."""
        return self._detect_batch(images, dev_ptrs, pitch)

    def getPoints(self, pos, score, level):
        """DetectorBaseGPU::processGrid (detector_base_gpu.cpp:204-218): the occupied cells as (x, y, score, level)."""
        occ = np.nonzero(score > 0)[0]
        return [(float(pos[i, 0]), float(pos[i, 1]), float(score[i]), int(level[i])) for i in occ]
