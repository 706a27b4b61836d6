"""What fastgrid.FASTGPU and harrisgrid.HarrisGPU share, as vilib's DetectorBaseGPU shares it: the handle, the grid size,
the pyramid and response read-backs and the marshalling of a batch, over the vslam_<prefix>_* functions of either C ABI."""
import ctypes as C

import numpy as np

from . import _check, _p, lib

_bound = set()


class GridDetector:
    _prefix = None  # "fg" | "hg"
    _n_extra = 0    # pointers that detect / detect_batch take behind pos, score, level

    def _fn(self, name):
        return getattr(self.L, "vslam_%s_%s" % (self._prefix, name))

    def _create(self, params, min_level, max_level):
        self._h = None  # before anything can raise: __del__ runs on a half-built object too
        self.L = lib()
        if self._prefix not in _bound:
            vp, i = C.c_void_p, C.c_int
            extra = [vp] * self._n_extra
            self._fn("create").argtypes = [C.POINTER(type(params)), C.POINTER(vp)]
            self._fn("destroy").argtypes = [vp]
            self._fn("destroy").restype = None
            self._fn("grid").argtypes = [vp, vp, vp]
            self._fn("detect").argtypes = [vp, vp, C.c_size_t, vp, vp, vp] + extra
            self._fn("detect_batch").argtypes = [vp, i, vp, C.c_size_t, i, vp, vp, vp] + extra
            self._fn("level_copy").argtypes = [vp, i, i, vp, C.c_size_t, vp, vp]
            self._fn("response_copy").argtypes = [vp, i, i, vp]
            _bound.add(self._prefix)
        h = C.c_void_p()
        _check(self._fn("create")(C.byref(params), C.byref(h)))
        self._h = h
        self.width, self.height, self.max_level, self.min_level = params.image_width, params.image_height, max_level, min_level
        nc, nr = C.c_int(), C.c_int()
        _check(self._fn("grid")(self._h, C.byref(nc), C.byref(nr)))
        self.n_cols, self.n_rows = nc.value, nr.value  # getCellCountHorizontal / getCellCountVertical
        self.cells = self.n_cols * self.n_rows

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _detect(self, image, *extra):
        """One host image -> (pos[cells, 2], score[cells], level[cells]); extra: the detector's own output pointers."""
        image = np.ascontiguousarray(image, np.uint8)
        assert image.shape == (self.height, self.width)
        pos = np.zeros((self.cells, 2), np.float32)
        sc = np.zeros(self.cells, np.float32)
        lv = np.zeros(self.cells, np.int32)
        _check(self._fn("detect")(self._h, _p(image), image.strides[0], _p(pos), _p(sc), _p(lv), *extra))
        return pos, sc, lv

    def _detect_batch(self, images, dev_ptrs, pitch, extra=lambda n: ()):
        """Host arrays, or device addresses (dev_ptrs, pitch) -> (pos[n, cells, 2], score[n, cells], level[n, cells]);
        extra(n): the detector's own output arrays."""
        if dev_ptrs is None:
            imgs = [np.ascontiguousarray(im, np.uint8) for im in images]
            n, pitch = len(imgs), imgs[0].strides[0]
            ptrs = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
            on_dev = 0
        else:
            n = len(dev_ptrs)
            ptrs = (C.c_void_p * n)(*dev_ptrs)
            on_dev = 1
        out = (np.zeros((n, self.cells, 2), np.float32), np.zeros((n, self.cells), np.float32),
               np.zeros((n, self.cells), np.int32)) + tuple(extra(n))
        _check(self._fn("detect_batch")(self._h, n, ptrs, pitch, on_dev, *[_p(a) for a in out]))
        return out

    def level(self, slot, level):
        w, h = C.c_int(), C.c_int()
        _check(self._fn("level_copy")(self._h, slot, level, None, 0, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        _check(self._fn("level_copy")(self._h, slot, level, _p(out), w.value, None, None))
        return out

    def response(self, slot, level):
        """DetectorBaseGPU::copyResponseTo (detector_base_gpu.cpp:127-141); 0 where the reference never writes."""
        out = np.zeros((self.height >> level, self.width >> level), np.float32)
        _check(self._fn("response_copy")(self._h, slot, level, _p(out)))
        return out
