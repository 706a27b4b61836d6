"""vilib::FeatureTrackerGPU over a FrameBundle of C cameras, restated with C unmodified lk_ref.Tracker objects -- the
yardstick of tests/test_gpu_featuretracker_bundle.py.  FeatureTrackerGPU::track (feature_tracker_gpu.cpp:85-288) runs each
of its steps in a loop over the cameras, and the cameras share nothing but the options, the detector and the track-id
counter (Point::getNewId, one counter per process; here one per tracker object, from 0).  Ids are only handed out in
step 03, which walks the cameras in order, so running the whole of camera 0's call before camera 1's gives the same ids:
the counter goes into a camera's book before its call and is read back afterwards."""
import lk_ref as lk


class BundleTracker:
    def __init__(self, opt, detect, n_cameras, n_cols, n_rows, cell_w=32, cell_h=32):
        self.T = [lk.Tracker(opt, detect, n_cols, n_rows, cell_w, cell_h) for _ in range(n_cameras)]
        self.next_id = 0

    def track(self, images):
        """one image per camera -> [(tracked, detected)] per camera"""
        assert len(images) == len(self.T)
        counts = []
        for T, img in zip(self.T, images):
            T.book.next_id = self.next_id
            counts.append(T.track(img))
            self.next_id = T.book.next_id
        return counts
