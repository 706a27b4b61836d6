"""Host-side mirror of the pyramidal Lucas-Kanade feature tracker, vilib::FeatureTrackerGPU
(thirdparty/vilib/visual_lib/src/feature_tracker/feature_tracker_gpu.cpp, feature_tracker_base.cpp) over the C ABI of
include/vslam_featuretracker.h.  The constructor takes vilib::FeatureTrackerOptions' fields and the bound detector
(setDetectorGPU): a fastgrid.FASTGPU or a harrisgrid.HarrisGPU, and how many cameras the object serves (a FrameBundle:
all of the detector's image size, at most its max_batch).  Book is the bookkeeping alone, from the GPU-free
libvslam_host.so."""
import ctypes as C

import numpy as np

from . import _check, _p, host_lib, lib

MAX_LEVELS = 8
DETECTOR_FAST, DETECTOR_HARRIS = 0, 1


class FtParams(C.Structure):  # vslam_ft_params
    _fields_ = [("klt_min_level", C.c_int32), ("klt_max_level", C.c_int32), ("klt_patch_sizes", C.c_int32 * MAX_LEVELS),
                ("klt_min_update_squared", C.c_float), ("min_tracks_to_detect_new_features", C.c_int32),
                ("reset_before_detection", C.c_int32), ("use_best_n_features", C.c_int32),
                ("klt_template_is_first_observation", C.c_int32), ("affine_est_offset", C.c_int32), ("affine_est_gain", C.c_int32),
                ("pyramid_levels", C.c_int32)]


class FtFeature(C.Structure):  # vslam_ft_feature
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("score", C.c_float), ("level", C.c_int32), ("track_id", C.c_int32)]


class FtTrackInfo(C.Structure):  # vslam_ft_track_info
    _fields_ = [("first_pos", C.c_float * 2), ("cur_pos", C.c_float * 2), ("cur_disparity", C.c_float), ("life", C.c_int32),
                ("track_id", C.c_int32), ("buffer_id", C.c_int32)]


FEATURE_DTYPE = np.dtype([("px", np.float32, 2), ("score", np.float32), ("level", np.int32), ("track_id", np.int32)])
TRACK_DTYPE = np.dtype([("first_pos", np.float32, 2), ("cur_pos", np.float32, 2), ("cur_disparity", np.float32), ("life", np.int32),
                        ("track_id", np.int32), ("buffer_id", np.int32)])
assert FEATURE_DTYPE.itemsize == C.sizeof(FtFeature) and TRACK_DTYPE.itemsize == C.sizeof(FtTrackInfo)


def make_params(klt_min_level=0, klt_max_level=4, klt_patch_sizes=(16, 16, 16, 8, 8), klt_min_update_squared=0.0005,
                min_tracks_to_detect_new_features=100, reset_before_detection=True, use_best_n_features=-1,
                klt_template_is_first_observation=True, affine_est_offset=False, affine_est_gain=False, pyramid_levels=5):
    """vilib::FeatureTrackerOptions' defaults (feature_tracker_options.h:50-98); pyramid_levels is Frame's n_pyr_levels"""
    sizes = list(klt_patch_sizes) + [0] * (MAX_LEVELS - len(klt_patch_sizes))
    return FtParams(klt_min_level, klt_max_level, (C.c_int32 * MAX_LEVELS)(*sizes[:MAX_LEVELS]), klt_min_update_squared,
                    min_tracks_to_detect_new_features, 1 if reset_before_detection else 0, use_best_n_features,
                    1 if klt_template_is_first_observation else 0, 1 if affine_est_offset else 0, 1 if affine_est_gain else 0,
                    pyramid_levels)


_bound = set()


def _bind(L, prefix):
    """signatures of the read side that vslam_ft_* and vslam_ftbook_* share"""
    key = (id(L), prefix)
    if key in _bound:
        return
    vp, i = C.c_void_p, C.c_int
    f = lambda name: getattr(L, "vslam_%s_%s" % (prefix, name))
    f("destroy").argtypes = [vp]
    f("destroy").restype = None
    f("capacity").argtypes = [vp]
    f("features").argtypes = [vp, vp, i, C.POINTER(i)]
    f("tracks").argtypes = [vp, vp, i, C.POINTER(i)]
    f("disparity").argtypes = [vp, C.c_double, C.POINTER(C.c_double)]
    f("reset").argtypes = [vp]
    f("set_best_n").argtypes = [vp, i]
    f("set_min_tracks").argtypes = [vp, i]
    if prefix == "ft":
        L.vslam_ft_create.argtypes = [C.POINTER(FtParams), i, vp, C.POINTER(vp)]
        L.vslam_ft_create_bundle.argtypes = [C.POINTER(FtParams), i, vp, i, C.POINTER(vp)]
        L.vslam_ft_cameras.argtypes = [vp]
        L.vslam_ft_track_bundle.argtypes = [vp, vp, C.c_size_t, i, vp, vp]
        L.vslam_ft_features_cam.argtypes = [vp, i, vp, i, C.POINTER(i)]
        L.vslam_ft_tracks_cam.argtypes = [vp, i, vp, i, C.POINTER(i)]
        L.vslam_ft_disparity_cam.argtypes = [vp, i, C.c_double, C.POINTER(C.c_double)]
        L.vslam_ft_template_copy_cam.argtypes = [vp, i, i, i, vp, vp]
        L.vslam_ft_track.argtypes = [vp, vp, C.c_size_t, i, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.vslam_ft_template_copy.argtypes = [vp, i, i, vp, vp]
        L.vslam_ft_profile.argtypes = [vp, i]
        L.vslam_ft_kernel_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    else:
        L.vslam_ftbook_create.argtypes = [C.POINTER(FtParams), i, i, i, i, C.POINTER(vp)]
        L.vslam_ftbook_results.argtypes = [vp, vp, i]
        L.vslam_ftbook_need_detect.argtypes = [vp]
        L.vslam_ftbook_detect.argtypes = [vp, vp, vp, vp, C.POINTER(i)]
        L.vslam_ftbook_update_count.argtypes = [vp]
        L.vslam_ftbook_next_id.argtypes = [vp]
        L.vslam_ftbook_set_next_id.argtypes = [vp, i]
    _bound.add(key)


class _ReadSide:
    _prefix = None

    def _fn(self, name):
        return getattr(self.L, "vslam_%s_%s" % (self._prefix, name))

    def _ok(self, rc):
        if self._prefix == "ft":
            _check(rc)
        elif rc != 0:
            raise ValueError("vslam_ftbook: invalid arguments")

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _cam(self, name, camera):
        """the function and its leading arguments; a tracker's read side names the camera, a book is one camera"""
        if self._prefix == "ft":
            return self._fn(name + "_cam"), (self._h, camera)
        if camera != 0:
            raise ValueError("vslam_ftbook: a book is one camera")
        return self._fn(name), (self._h,)

    def _list(self, name, dtype, camera):
        out = np.zeros(self.capacity, dtype)
        n = C.c_int()
        f, head = self._cam(name, camera)
        self._ok(f(*head, _p(out), self.capacity, C.byref(n)))
        return out[:n.value]

    def features(self, camera=0):
        """the frame's feature list in addFeature order: px, score, level, track_id"""
        return self._list("features", FEATURE_DTYPE, camera)

    def tracks(self, camera=0):
        """the live tracks: first_pos, cur_pos, cur_disparity, life, track_id, buffer_id"""
        return self._list("tracks", TRACK_DTYPE, camera)

    def getDisparity(self, pivot_ratio, camera=0):
        d = C.c_double()
        f, head = self._cam("disparity", camera)
        self._ok(f(*head, pivot_ratio, C.byref(d)))
        return d.value

    def reset(self):
        self._ok(self._fn("reset")(self._h))

    def setBestNFeatures(self, n):
        self._ok(self._fn("set_best_n")(self._h, n))

    def setMinTracksToDetect(self, n):
        self._ok(self._fn("set_min_tracks")(self._h, n))


class FeatureTrackerGPU(_ReadSide):
    """vilib::FeatureTrackerGPU(options, cameras) + setDetectorGPU(detector, c) for every camera c: the cameras share the
    detector (image size, grid, stream; cameras <= its max_batch) and the options, and nothing else but the track-id counter.
    Keep the detector alive as long as the tracker.  capacity is per camera."""
    _prefix = "ft"

    def __init__(self, detector, cameras=1, **options):
        self._h = None
        self.L = lib()
        _bind(self.L, "ft")
        self.detector = detector
        self.params = make_params(**options)
        h = C.c_void_p()
        kind = DETECTOR_HARRIS if detector._prefix == "hg" else DETECTOR_FAST
        _check(self.L.vslam_ft_create_bundle(C.byref(self.params), kind, detector._h, cameras, C.byref(h)))
        self._h = h
        self.capacity = self.L.vslam_ft_capacity(h)
        self.cameras = self.L.vslam_ft_cameras(h)

    def track(self, image=None, dev_ptr=None, pitch=None):
        """FeatureTrackerGPU::track on one frame: a host array, or a device address (dev_ptr, pitch) -> (n_tracked, n_detected)"""
        nt, nd = C.c_int32(), C.c_int32()
        if dev_ptr is None:
            image = np.ascontiguousarray(image, np.uint8)
            assert image.shape == (self.detector.height, self.detector.width)
            _check(self.L.vslam_ft_track(self._h, _p(image), image.strides[0], 0, C.byref(nt), C.byref(nd)))
        else:
            _check(self.L.vslam_ft_track(self._h, C.c_void_p(dev_ptr), pitch, 1, C.byref(nt), C.byref(nd)))
        return nt.value, nd.value

    def track_bundle(self, images=None, dev_ptrs=None, pitch=None):
        """FeatureTrackerGPU::track on a FrameBundle: one host array per camera, or one device address per camera
        (dev_ptrs, pitch) -> [(n_tracked, n_detected)] per camera"""
        n = self.cameras
        nt, nd = np.zeros(n, np.int32), np.zeros(n, np.int32)
        if dev_ptrs is None:
            images = [np.ascontiguousarray(im, np.uint8) for im in images]
            assert len(images) == n and all(im.shape == (self.detector.height, self.detector.width) for im in images)
            ptrs = (C.c_void_p * n)(*[im.ctypes.data for im in images])
            _check(self.L.vslam_ft_track_bundle(self._h, ptrs, images[0].strides[0], 0, _p(nt), _p(nd)))
        else:
            assert len(dev_ptrs) == n
            ptrs = (C.c_void_p * n)(*dev_ptrs)
            _check(self.L.vslam_ft_track_bundle(self._h, ptrs, pitch, 1, _p(nt), _p(nd)))
        return [(int(a), int(b)) for a, b in zip(nt, nd)]

    def profile(self, enable=True):
        """diagnostic: bracket the two kernels of every track() with HIP events"""
        _check(self.L.vslam_ft_profile(self._h, 1 if enable else 0))

    def kernel_ms(self):
        """(k_ft_track, k_ft_update) milliseconds of the last track() after profile()"""
        a, b = C.c_float(), C.c_float()
        _check(self.L.vslam_ft_kernel_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def template(self, track, level, camera=0):
        """diagnostic: (patch[(ps+2), (ps+2)] int32, invH[10] float32) of camera `camera`'s live track `track` on pyramid level `level`"""
        side = self.params.klt_patch_sizes[level] + 2
        patch, inv = np.zeros((side, side), np.int32), np.zeros(10, np.float32)
        _check(self.L.vslam_ft_template_copy_cam(self._h, camera, track, level, _p(patch), _p(inv)))
        return patch, inv


class Book(_ReadSide):
    """vslam_ftbook: steps 02 and 03 of FeatureTrackerGPU::track without the kernels (libvslam_host.so)."""
    _prefix = "ftbook"

    def __init__(self, n_cols, n_rows, cell_w=32, cell_h=32, **options):
        self._h = None
        self.L = host_lib()
        _bind(self.L, "ftbook")
        self.params = make_params(**options)
        h = C.c_void_p()
        self._ok(self.L.vslam_ftbook_create(C.byref(self.params), n_cols, n_rows, cell_w, cell_h, C.byref(h)))
        self._h = h
        self.capacity = self.L.vslam_ftbook_capacity(h)

    def results(self, res):
        res = np.ascontiguousarray(res, np.float32).reshape(-1, 4)
        self._ok(self.L.vslam_ftbook_results(self._h, _p(res), len(res)))

    def need_detect(self):
        return bool(self.L.vslam_ftbook_need_detect(self._h))

    def detect(self, pos, score, level):
        n = C.c_int()
        pos, score, level = np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(score, np.float32), np.ascontiguousarray(level, np.int32)
        self._ok(self.L.vslam_ftbook_detect(self._h, _p(pos), _p(score), _p(level), C.byref(n)))
        return n.value

    def update_count(self):
        return self.L.vslam_ftbook_update_count(self._h)

    @property
    def next_id(self):
        """the id the next new track gets; a tracker over several books threads one counter through them"""
        return self.L.vslam_ftbook_next_id(self._h)

    @next_id.setter
    def next_id(self, value):
        self._ok(self.L.vslam_ftbook_set_next_id(self._h, value))
