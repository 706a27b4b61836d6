"""Host-side mirror of the grid Harris / Shi-Tomasi detector, vilib::HarrisGPU
(thirdparty/vilib/visual_lib/src/feature_detection/harris/harris_gpu.cpp:63-207) over the C ABI of
include/vslam_harrisgrid.h.  Same constructor arguments, same feature grid, the sibling of fastgrid.FASTGPU."""
import ctypes as C

import numpy as np

from . import _check, _p, lib

# vilib::conv_filter_border_type (preprocess/conv_filter.h:59-72)
BORDER_SKIP, BORDER_ZERO, BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101 = range(6)


class _HgParams(C.Structure):  # vslam_hg_params
    _fields_ = [("image_width", C.c_int32), ("image_height", C.c_int32), ("cell_size_width", C.c_int32),
                ("cell_size_height", C.c_int32), ("min_level", C.c_int32), ("max_level", C.c_int32),
                ("horizontal_border", C.c_int32), ("vertical_border", C.c_int32), ("filter_border_type", C.c_int32),
                ("use_harris", C.c_int32), ("harris_k", C.c_float), ("quality_level", C.c_float), ("tie_rule", C.c_int32),
                ("device", C.c_int32), ("max_batch", C.c_int32)]


_bound = False


def _bind():
    global _bound
    L = lib()
    if not _bound:
        vp, i = C.c_void_p, C.c_int
        L.vslam_hg_create.argtypes = [C.POINTER(_HgParams), C.POINTER(vp)]
        L.vslam_hg_destroy.argtypes = [vp]
        L.vslam_hg_destroy.restype = None
        L.vslam_hg_grid.argtypes = [vp, vp, vp]
        L.vslam_hg_detect.argtypes = [vp, vp, C.c_size_t, vp, vp, vp, vp, vp]
        L.vslam_hg_detect_batch.argtypes = [vp, i, vp, C.c_size_t, i, vp, vp, vp, vp, vp]
        L.vslam_hg_level_copy.argtypes = [vp, i, i, vp, C.c_size_t, vp, vp]
        L.vslam_hg_response_copy.argtypes = [vp, i, i, vp]
        _bound = True
    return L


class HarrisGPU:
    """vilib::HarrisGPU(image_width, image_height, cell_size_width, cell_size_height, min_level, max_level,
    horizontal_border, vertical_border, filter_border_type, use_harris, harris_k, quality_level) (harris_gpu.cpp:63-98)."""

    def __init__(self, image_width, image_height, cell_size_width=32, cell_size_height=32, min_level=0, max_level=1,
                 horizontal_border=0, vertical_border=0, filter_border_type=BORDER_SKIP, use_harris=True, harris_k=0.04,
                 quality_level=0.1, tie_rule=0, device=0, max_batch=1):
        self.L = _bind()
        self._h = None
        P = _HgParams(image_width, image_height, cell_size_width, cell_size_height, min_level, max_level,
                      horizontal_border, vertical_border, filter_border_type, 1 if use_harris else 0, harris_k,
                      quality_level, tie_rule, device, max_batch)
        h = C.c_void_p()
        _check(self.L.vslam_hg_create(C.byref(P), C.byref(h)))
        self._h = h
        self.width, self.height, self.max_level, self.min_level = image_width, image_height, max_level, min_level
        nc, nr = C.c_int(), C.c_int()
        _check(self.L.vslam_hg_grid(self._h, C.byref(nc), C.byref(nr)))
        self.n_cols, self.n_rows = nc.value, nr.value  # getCellCountHorizontal / getCellCountVertical
        self.cells = self.n_cols * self.n_rows

    def close(self):
        if self._h:
            self.L.vslam_hg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def detect(self, image, raw=False):
        """Frame(image) + HarrisGPU::detect -> (pos[cells, 2], score[cells], level[cells], keep[cells], n_keep);
        raw=True is the callback overload: the grid alone, no threshold step."""
        image = np.ascontiguousarray(image, np.uint8)
        assert image.shape == (self.height, self.width)
        pos = np.zeros((self.cells, 2), np.float32)
        sc = np.zeros(self.cells, np.float32)
        lv = np.zeros(self.cells, np.int32)
        if raw:
            _check(self.L.vslam_hg_detect(self._h, _p(image), image.strides[0], _p(pos), _p(sc), _p(lv), None, None))
            return pos, sc, lv
        keep = np.zeros(self.cells, np.uint8)
        nk = C.c_int32(0)
        _check(self.L.vslam_hg_detect(self._h, _p(image), image.strides[0], _p(pos), _p(sc), _p(lv), _p(keep), C.byref(nk)))
        return pos, sc, lv, keep.astype(bool), nk.value

    def detect_batch(self, images=None, dev_ptrs=None, pitch=None):
        """Several images per pass: host arrays, or device addresses (dev_ptrs, pitch).  The threshold is per image."""
        if dev_ptrs is None:
            imgs = [np.ascontiguousarray(im, np.uint8) for im in images]
            n, pitch = len(imgs), imgs[0].strides[0]
            ptrs = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
            on_dev = 0
        else:
            n = len(dev_ptrs)
            ptrs = (C.c_void_p * n)(*dev_ptrs)
            on_dev = 1
        pos = np.zeros((n, self.cells, 2), np.float32)
        sc = np.zeros((n, self.cells), np.float32)
        lv = np.zeros((n, self.cells), np.int32)
        keep = np.zeros((n, self.cells), np.uint8)
        nk = np.zeros(n, np.int32)
        _check(self.L.vslam_hg_detect_batch(self._h, n, ptrs, pitch, on_dev, _p(pos), _p(sc), _p(lv), _p(keep), _p(nk)))
        return pos, sc, lv, keep.astype(bool), nk

    def getPoints(self, pos, score, level, keep, n_keep=None):
        """DetectorBaseGPU::processGridAndThreshold (detector_base_gpu.cpp:228-248): the kept cells as (x, y, score, level)."""
        return [(float(pos[i, 0]), float(pos[i, 1]), float(score[i]), int(level[i])) for i in np.nonzero(keep)[0]]

    def level(self, slot, level):
        w, h = C.c_int(), C.c_int()
        _check(self.L.vslam_hg_level_copy(self._h, slot, level, None, 0, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        _check(self.L.vslam_hg_level_copy(self._h, slot, level, _p(out), w.value, None, None))
        return out

    def response(self, slot, level):
        """DetectorBaseGPU::copyResponseTo (detector_base_gpu.cpp:127-141); 0 where the reference never writes."""
        out = np.zeros((self.height >> level, self.width >> level), np.float32)
        _check(self.L.vslam_hg_response_copy(self._h, slot, level, _p(out)))
        return out
