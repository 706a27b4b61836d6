"""Host-side mirror of the grid Harris / Shi-Tomasi detector, vilib::HarrisGPU
(thirdparty/vilib/visual_lib/src/feature_detection/harris/harris_gpu.cpp:63-207) over the C ABI of
include/vslam_harrisgrid.h.  Same constructor arguments, same feature grid, the sibling of fastgrid.FASTGPU."""
import ctypes as C

import numpy as np

from . import _p
from ._griddet import GridDetector

# vilib::conv_filter_border_type (preprocess/conv_filter.h:59-72)
BORDER_SKIP, BORDER_ZERO, BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101 = range(6)


class _HgParams(C.Structure):  # vslam_hg_params
    _fields_ = [("image_width", C.c_int32), ("image_height", C.c_int32), ("cell_size_width", C.c_int32),
                ("cell_size_height", C.c_int32), ("min_level", C.c_int32), ("max_level", C.c_int32),
                ("horizontal_border", C.c_int32), ("vertical_border", C.c_int32), ("filter_border_type", C.c_int32),
                ("use_harris", C.c_int32), ("harris_k", C.c_float), ("quality_level", C.c_float), ("tie_rule", C.c_int32),
                ("device", C.c_int32), ("max_batch", C.c_int32)]


class HarrisGPU(GridDetector):
    """vilib::HarrisGPU(image_width, image_height, cell_size_width, cell_size_height, min_level, max_level,
    horizontal_border, vertical_border, filter_border_type, use_harris, harris_k, quality_level) (harris_gpu.cpp:63-98)."""
    _prefix, _n_extra = "hg", 2  # keep, n_keep

    def __init__(self, image_width, image_height, cell_size_width=32, cell_size_height=32, min_level=0, max_level=1,
                 horizontal_border=0, vertical_border=0, filter_border_type=BORDER_SKIP, use_harris=True, harris_k=0.04,
                 quality_level=0.1, tie_rule=0, device=0, max_batch=1):
        self._create(_HgParams(image_width, image_height, cell_size_width, cell_size_height, min_level, max_level,
                               horizontal_border, vertical_border, filter_border_type, 1 if use_harris else 0, harris_k,
                               quality_level, tie_rule, device, max_batch), min_level, max_level)

    def detect(self, image, raw=False):
        """Frame(image) + HarrisGPU::detect -> (pos[cells, 2], score[cells], level[cells], keep[cells], n_keep);
        raw=True is the callback overload: the grid alone, no threshold step."""
        if raw:
            return self._detect(image, None, None)
        keep = np.zeros(self.cells, np.uint8)
        nk = C.c_int32(0)
        return self._detect(image, _p(keep), C.byref(nk)) + (keep.astype(bool), nk.value)

    def detect_batch(self, images=None, dev_ptrs=None, pitch=None):
        """Several images per pass: host arrays, or device addresses (dev_ptrs, pitch).  The threshold is per image."""
        pos, sc, lv, keep, nk = self._detect_batch(images, dev_ptrs, pitch,
                                                   lambda n: (np.zeros((n, self.cells), np.uint8), np.zeros(n, np.int32)))
        return pos, sc, lv, keep.astype(bool), nk

    def getPoints(self, pos, score, level, keep, n_keep=None):
        """DetectorBaseGPU::processGridAndThreshold (detector_base_gpu.cpp:228-248): the kept cells as (x, y, score, level)."""
        return [(float(pos[i, 0]), float(pos[i, 1]), float(score[i]), int(level[i])) for i in np.nonzero(keep)[0]]
