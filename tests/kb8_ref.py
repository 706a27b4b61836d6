"""CPU reference for the fisheye camera (KannalaBrandt8): numpy float32 restatements, written from the sources and not from
vi_slam_amd/csrc/vslam_kb8.h, of

  * glibc 2.35 atanf, atan2f, tanf (|x| < 3*pi/4), sinf, cosf          sysdeps/ieee754/flt-32/{s_atanf,e_atan2f,k_tanf,s_tanf}.c,
                                                                       s_sincosf.h
  * KannalaBrandt8::project / unproject                                kannalabrandt8.cpp:11-27, :82-109
  * Frame::isInFrustum with the virtual camera, Nleft == -1            frame.cpp:529-595
  * Frame::isInFrustum of a two-camera rig, isInFrustumChecks          frame.cpp:596-606, :1191-1271

np.float32 array operations are IEEE operations without contraction.  The libm functions are vectorised (the tests compare
millions of arguments): every branch of the C text is evaluated for every element and np.where picks, in the C text's order
of tests.  The frustum part reuses tests/frustum_ref.py (Matx accumulation, cv::norm, PredictScale, records).
"""
import math

import numpy as np

import frustum_ref as FR

F32, F64, U32, I32 = np.float32, np.float64, np.uint32, np.int32


def _f(a):
    return np.ascontiguousarray(a, F32)


def _bits(a):
    return _f(a).view(U32)


def _from_bits(u):
    return np.ascontiguousarray(u, U32).view(F32)


# ---------------------------------------------------------------------------------------------- atanf (s_atanf.c)
_ATANHI = [F32(v) for v in (4.6364760399e-01, 7.8539812565e-01, 9.8279368877e-01, 1.5707962513e+00)]
_ATANLO = [F32(v) for v in (5.0121582440e-09, 3.7748947079e-08, 3.4473217170e-08, 7.5497894159e-08)]
_AT = [F32(v) for v in (3.3333334327e-01, -2.0000000298e-01, 1.4285714924e-01, -1.1111110449e-01, 9.0908870101e-02,
                        -7.6918758452e-02, 6.6610731184e-02, -5.8335702866e-02, 4.9768779427e-02, -3.6531571299e-02,
                        1.6285819933e-02)]
ONE, TWO = F32(1), F32(2)


def atanf(x):
    x = _f(x)
    with np.errstate(all="ignore"):
        hx = x.view(I32)
        ix = hx & I32(0x7fffffff)
        ax = np.abs(x)
        red = [(TWO * ax - ONE) / (TWO + ax), (ax - ONE) / (ax + ONE), (ax - F32(1.5)) / (ONE + F32(1.5) * ax), -ONE / ax]
        idn = np.where(ix < 0x3ee00000, -1, np.where(ix < 0x3f300000, 0, np.where(ix < 0x3f980000, 1,
                                                                                  np.where(ix < 0x401c0000, 2, 3))))
        t = x.copy()
        hi, lo = np.zeros_like(x), np.zeros_like(x)
        for k in range(4):
            t = np.where(idn == k, red[k], t)
            hi = np.where(idn == k, _ATANHI[k], hi)
            lo = np.where(idn == k, _ATANLO[k], lo)
        z = t * t
        w = z * z
        s1 = z * (_AT[0] + w * (_AT[2] + w * (_AT[4] + w * (_AT[6] + w * (_AT[8] + w * _AT[10])))))
        s2 = w * (_AT[1] + w * (_AT[3] + w * (_AT[5] + w * (_AT[7] + w * _AT[9]))))
        small = t - t * (s1 + s2)
        zz = hi - ((t * (s1 + s2) - lo) - t)
        gen = np.where(hx < 0, -zz, zz)
        out = np.where(idn < 0, small, gen)
        out = np.where((idn < 0) & (ix < 0x31000000), x, out)
        big = _ATANHI[3] + _ATANLO[3]
        out = np.where(ix >= 0x4c000000, np.where(hx > 0, big, -big), out)
        out = np.where(ix > 0x7f800000, x + x, out)
    return out.astype(F32)


# ---------------------------------------------------------------------------------------------- atan2f (e_atan2f.c)
_TINY, _PI_O_4, _PI_O_2, _PI, _PI_LO = (F32(v) for v in (1.0e-30, 7.8539818525e-01, 1.5707963705e+00, 3.1415927410e+00,
                                                          -8.7422776573e-08))


def atan2f(y, x):
    y, x = np.broadcast_arrays(_f(y), _f(x))
    y, x = _f(y), _f(x)
    with np.errstate(all="ignore"):
        hx, hy = x.view(I32), y.view(I32)
        ix, iy = hx & I32(0x7fffffff), hy & I32(0x7fffffff)
        m = ((hy >> 31) & 1) | ((hx >> 30) & 2)
        k = (iy - ix) >> 23
        z = np.where(k > 60, _PI_O_2 + F32(0.5) * _PI_LO, np.where((hx < 0) & (k < -60), F32(0), atanf(np.abs(y / x))))
        z = z.astype(F32)
        by_m = [z, _from_bits(_bits(z) ^ U32(0x80000000)), _PI - (z - _PI_LO), (z - _PI_LO) - _PI]
        out = np.select([m == 0, m == 1, m == 2], by_m[:3], by_m[3])
        inf = I32(0x7f800000)
        y_inf = np.where(hy < 0, -_PI_O_2 - _TINY, _PI_O_2 + _TINY)
        out = np.where(iy == inf, y_inf, out)
        both = np.select([m == 0, m == 1, m == 2],
                         [_PI_O_4 + _TINY, -_PI_O_4 - _TINY, F32(3.0) * _PI_O_4 + _TINY], F32(-3.0) * _PI_O_4 - _TINY)
        xinf = np.select([m == 0, m == 1, m == 2], [F32(0.0), F32(-0.0), _PI + _TINY], -_PI - _TINY)
        out = np.where(ix == inf, np.where(iy == inf, both, xinf), out)
        out = np.where(ix == 0, y_inf, out)
        y0 = np.select([m < 2, m == 2], [y, _PI + _TINY], -_PI - _TINY)
        out = np.where(iy == 0, y0, out)
        out = np.where(hx == 0x3f800000, atanf(y), out)
        out = np.where((ix > inf) | (iy > inf), x + y, out)
    return out.astype(F32)


def atan2f_correctly_rounded(y, x):
    """float(atan2(double, double)): what a correctly rounded libm returns -- NOT glibc's; for the sensitivity condition"""
    return np.arctan2(_f(y).astype(F64), _f(x).astype(F64)).astype(F32)


# ---------------------------------------------------------------------------------------------- tanf (k_tanf.c, s_tanf.c)
_T = [F32(v) for v in (3.3333334327e-01, 1.3333334029e-01, 5.3968254477e-02, 2.1869488060e-02, 8.8632395491e-03,
                       3.5920790397e-03, 1.4562094584e-03, 5.8804126456e-04, 2.4646313977e-04, 7.8179444245e-05,
                       7.1407252108e-05, -1.8558637748e-05, 2.5907305826e-05)]
_PIO4, _PIO4LO = F32(7.8539812565e-01), F32(3.7748947079e-08)


def _kernel_tanf(x, y, iy):
    """__kernel_tanf(x, y, iy) elementwise; iy an int array of 1 / -1"""
    hx = x.view(I32)
    ix = hx & I32(0x7fffffff)
    iyf = iy.astype(F32)
    sgn = (1 - ((hx >> 30) & 2)).astype(F32)
    tiny = ix < 0x39000000
    r_tiny = np.where((ix | (iy + 1)) == 0, ONE / np.abs(x), np.where(iy == 1, x, (-1.0 / x.astype(F64)).astype(F32)))
    big = ix >= 0x3f2ca140
    xn, yn = np.where(hx < 0, -x, x), np.where(hx < 0, -y, y)
    xb = (_PIO4 - xn) + (_PIO4LO - yn)
    x1 = np.where(big, xb, x).astype(F32)
    y1 = np.where(big, F32(0), y).astype(F32)
    early = big & (np.abs(x1) < F32(2.0 ** -13))
    r_early = (sgn * iyf) * (ONE - (TWO * iyf) * x1)
    z = x1 * x1
    w = z * z
    r = _T[1] + w * (_T[3] + w * (_T[5] + w * (_T[7] + w * (_T[9] + w * _T[11]))))
    v = z * (_T[2] + w * (_T[4] + w * (_T[6] + w * (_T[8] + w * (_T[10] + w * _T[12])))))
    s = z * x1
    r = y1 + z * (s * (r + v) + y1)
    r = r + _T[0] * s
    w = x1 + r
    r_big = sgn * (iyf - TWO * (x1 - (w * w / (w + iyf) - r)))
    zz = _from_bits(_bits(w) & U32(0xfffff000))
    vv = r - (zz - x1)
    a = -ONE / w
    t = _from_bits(_bits(a) & U32(0xfffff000))
    ss = ONE + t * zz
    r_neg = t + a * (ss + t * vv)
    out = np.where(big, r_big, np.where(iy == 1, w, r_neg))
    out = np.where(early, r_early, out)
    return np.where(tiny, r_tiny, out).astype(F32)


def tanf(x):
    """glibc tanf for |x| < 3*pi/4; NaN beyond (not restated)"""
    x = _f(x)
    with np.errstate(all="ignore"):
        ix = x.view(I32) & I32(0x7fffffff)
        direct = _kernel_tanf(x, np.zeros_like(x), np.ones(x.shape, I32))
        pio2 = 1.57079632679489661923
        r = x.astype(F64) + np.where(x.view(I32) < 0, pio2, -pio2)
        y0 = r.astype(F32)
        y1 = (r - y0.astype(F64)).astype(F32)
        reduced = _kernel_tanf(y0, y1, np.full(x.shape, -1, I32))
        out = np.where(ix <= 0x3f490fda, direct, reduced)
        out = np.where(ix >= 0x4016cbe4, F32(np.nan), out)
    return out.astype(F32)


# ---------------------------------------------------------------------------------------------- sinf / cosf (s_sincosf.h)
_HPI_INV, _HPI = float.fromhex("0x1.45F306DC9C883p+23"), float.fromhex("0x1.921FB54442D18p0")
_C = [float.fromhex(h) for h in ("0x1p0", "-0x1.ffffffd0c621cp-2", "0x1.55553e1068f19p-5", "-0x1.6c087e89a359dp-10",
                                 "0x1.99343027bf8c3p-16")]
_S = [float.fromhex(h) for h in ("-0x1.555545995a603p-3", "0x1.1107605230bc4p-7", "-0x1.994eb3774cf24p-13")]


def _sincosf(y, cos):
    y = _f(y)
    with np.errstate(all="ignore"):
        top = (y.view(U32) >> U32(20)) & U32(0x7ff)
        x = y.astype(F64)
        small, tiny, mid = top < 0x3f4, top < 0x398, top < 0x42f
        r = np.where(mid & ~small, x * _HPI_INV, 0.0)
        n = (r.astype(I32) + I32(0x800000)) >> 24
        xr = np.where(small, x, x - n * _HPI)
        sign = np.where(((n & 3) == 1) | ((n & 3) == 2), -1.0, 1.0)
        xs = xr * sign
        neg = (n & 2) != 0
        nn = n ^ 1 if cos else n
        x2 = xr * xr
        x3 = xs * x2
        s1 = _S[1] + x2 * _S[2]
        x7 = x3 * x2
        s = xs + x3 * _S[0]
        sine = (s + x7 * s1).astype(F32)
        sg = np.where(neg, -1.0, 1.0)
        x4 = x2 * x2
        c2 = sg * _C[3] + x2 * (sg * _C[4])
        c1 = sg * _C[0] + x2 * (sg * _C[1])
        x6 = x4 * x2
        c = c1 + x4 * (sg * _C[2])
        cosine = (c + x6 * c2).astype(F32)
        out = np.where((nn & 1) == 0, sine, cosine)
        out = np.where(tiny, F32(1) if cos else y, out)
        out = np.where(mid, out, F32(np.nan))
    return out.astype(F32)


def sinf(y):
    """glibc sinf for |y| < 120"""
    return _sincosf(y, False)


def cosf(y):
    return _sincosf(y, True)


# ---------------------------------------------------------------------------------------------- the camera
def camera(fx, fy, cx, cy, k, precision=0.0):
    return dict(fx=F32(fx), fy=F32(fy), cx=F32(cx), cy=F32(cy), k=[F32(v) for v in k], precision=F32(precision))


def project(cam, xyz, atan2=atan2f):
    """kannalabrandt8.cpp:11-27 over n x 3 points -> n x 2; `atan2` replaces the libm function (sensitivity condition)"""
    p = _f(xyz).reshape(-1, 3)
    x, y, z = _f(p[:, 0]), _f(p[:, 1]), _f(p[:, 2])
    k = cam["k"]
    with np.errstate(all="ignore"):
        x2y2 = x * x + y * y
        theta = atan2(np.sqrt(x2y2), z)
        psi = atan2(y, x)
        t2 = theta * theta
        t3 = theta * t2
        t5 = t3 * t2
        t7 = t5 * t2
        t9 = t7 * t2
        r = theta + k[0] * t3 + k[1] * t5 + k[2] * t7 + k[3] * t9
        u = cam["fx"] * r * cosf(psi) + cam["cx"]
        v = cam["fy"] * r * sinf(psi) + cam["cy"]
    return np.stack([u, v], 1).astype(F32)


def unproject(cam, uv):
    """kannalabrandt8.cpp:82-109 over n x 2 pixels -> (n x 3 rays, Newton steps per pixel [0: the guard failed], the largest
    |theta| the loop held per pixel)"""
    p = _f(uv).reshape(-1, 2)
    prec = cam["precision"] if cam["precision"] > 0 else F32(1e-6)
    k = cam["k"]
    pio2 = F32(math.pi / 2)
    with np.errstate(all="ignore"):
        pwx = (_f(p[:, 0]) - cam["cx"]) / cam["fx"]
        pwy = (_f(p[:, 1]) - cam["cy"]) / cam["fy"]
        theta_d = np.sqrt(pwx * pwx + pwy * pwy)
        theta_d = np.where(np.isnan(theta_d) | (theta_d < -pio2), -pio2, theta_d)  # fmaxf(-pi/2, theta_d)
        theta_d = np.where(theta_d > pio2, pio2, theta_d).astype(F32)              # fminf(.., pi/2)
        guard = theta_d.astype(F64) > 1e-8
        theta = theta_d.copy()
        active = guard.copy()
        steps = np.zeros(len(p), I32)
        tmax = np.abs(theta_d)
        for j in range(10):
            th2 = theta * theta
            th4 = th2 * th2
            th6 = th4 * th2
            th8 = th4 * th4
            k0, k1, k2, k3 = k[0] * th2, k[1] * th4, k[2] * th6, k[3] * th8
            fix = (theta * (ONE + k0 + k1 + k2 + k3) - theta_d) / (ONE + F32(3) * k0 + F32(5) * k1 + F32(7) * k2 + F32(9) * k3)
            theta = np.where(active, theta - fix, theta).astype(F32)
            steps = np.where(active, j + 1, steps)
            tmax = np.where(active, np.maximum(tmax, np.abs(theta)), tmax)
            active = active & ~(np.abs(fix) < prec)
        scale = np.where(guard, tanf(theta) / theta_d, ONE).astype(F32)
        out = np.stack([pwx * scale, pwy * scale, np.ones_like(scale)], 1)
    return out.astype(F32), steps, tmax


# ---------------------------------------------------------------------------------------------- frustum
#: the exits of frame.cpp:529-595 as FR.in_frustum names them
EXITS = FR.EXITS


def _transform(T, pos):
    """Matx product rows and the Matx addition, float accumulation from zero, over n points"""
    T = np.asarray(T, F32).reshape(3, 4)
    X = _f(pos).reshape(-1, 3)
    out = []
    with np.errstate(all="ignore"):
        for r in range(3):
            s = np.zeros(len(X), F32)
            for c in range(3):
                s = s + T[r, c] * _f(X[:, c])
            out.append(s + T[r, 3])
    return np.stack(out, 1).astype(F32)


def _after_bounds(P, mp, twc, u, v, det):
    """frame.cpp:560-580 / :1235-1253: -> (exit name, dist, view_cos, level)"""
    Px = np.asarray(mp["pos"], F32)
    PO = [F32(Px[k] - F32(twc[k])) for k in range(3)]
    dist = FR._norm(PO)
    det["dist"] = dist
    if dist < F32(mp["min_dist"]):
        return "too_close", dist, F32(0), 0
    if dist > F32(mp["max_dist"]):
        return "too_far", dist, F32(0), 0
    with np.errstate(all="ignore"):
        view_cos = F32(FR._acc3(PO, np.asarray(mp["normal"], F32), False) / dist)
    det["view_cos"] = view_cos
    if view_cos < F32(P["viewing_cos_limit"]):
        return "view_cos", dist, view_cos, 0
    return "in_view", dist, view_cos, FR.predict_scale(mp["max_dist"], dist, P["log_scale_factor"], det["nlevels"])


def frame_in_frustum(P, cam, points, bounds, nlevels, atan2=atan2f):
    """Frame::isInFrustum, Nleft == -1, mpCamera = KannalaBrandt8 -> the tuple of FR.frame_in_frustum"""
    from oracle import orbo
    n = len(points)
    track = np.zeros(n, orbo.MP_TRACK_DTYPE)
    depth = np.zeros(n, F32)
    exits, dets = [], []
    Pc = _transform(P["Tcw"], points["pos"])
    uv = project(cam, Pc, atan2)
    b = [F32(x) for x in bounds]
    for i in range(n):
        mp = points[i]
        fl = int(mp["flags"])
        keep2 = fl & 2
        rec, d, why, det = (F32(-1), F32(-1), F32(0), F32(0), 0, keep2), F32(0), None, {}
        z = Pc[i, 2]
        u, v = uv[i]
        if not fl & 1:
            why = "not_candidate"
        elif z < F32(0):
            why = "behind"
        else:
            det = dict(u=u, v=v, z=z, nlevels=nlevels)
            if u < b[0]:
                why = "left"
            elif u > b[1]:
                why = "right"
            elif v < b[2]:
                why = "top"
            elif v > b[3]:
                why = "bottom"
            else:
                rec = (u, v, F32(0), F32(0), 0, keep2)  # :557-558
                why, dist, vc, level = _after_bounds(P, mp, P["Ow"], u, v, det)
                if why == "in_view":
                    with np.errstate(all="ignore"):
                        invz = F32(F32(1.0) / z)
                        xr = F32(u - F32(F32(P["mbf"]) * invz))
                    rec = (u, v, xr, vc, level, keep2 | 1)
                    d = FR._norm(Pc[i])
        track[i] = rec
        depth[i] = d
        exits.append(why)
        dets.append(det)
    return track, depth, int((track["flags"] & 1).sum()), exits, dets


def rig_right_pose(P, rig):
    """isInFrustumChecks, bRight: mRx = Rrl * Rcw, mtx = Rrl * tcw + trl with tcw = mOwx (as written), twcx = Rwc * tlr + tcw"""
    T = np.asarray(P["Tcw"], F32).reshape(3, 4)
    Ow = np.asarray(P["Ow"], F32)
    Trl, Tlr = np.asarray(rig["Trl"], F32).reshape(3, 4), np.asarray(rig["Tlr"], F32).reshape(3, 4)
    M = np.zeros((3, 4), F32)
    for i in range(3):
        for j in range(3):
            M[i, j] = FR._acc3(Trl[i, :3], T[:, j], False)
        M[i, 3] = F32(FR._acc3(Trl[i, :3], Ow, False) + Trl[i, 3])
    twc = [F32(FR._acc3(T[:, i], Tlr[:, 3], False) + Ow[i]) for i in range(3)]
    return M, np.array(twc, F32)


def _checks(P, cam, T, twc, points, bounds, nlevels):
    from oracle import orbo
    n = len(points)
    track = np.zeros(n, orbo.MP_TRACK_DTYPE)
    track["level"] = -1
    depth = np.zeros(n, F32)
    Pc = _transform(T, points["pos"])
    uv = project(cam, Pc)
    b = [F32(x) for x in bounds]
    for i in range(n):
        mp = points[i]
        fl = int(mp["flags"])
        track["flags"][i] = fl & 2
        u, v = uv[i]
        if not fl & 1 or Pc[i, 2] < F32(0) or u < b[0] or u > b[1] or v < b[2] or v > b[3]:
            continue
        why, dist, vc, level = _after_bounds(P, mp, twc, u, v, dict(nlevels=nlevels))
        if why != "in_view":
            continue
        track[i] = (u, v, F32(0), vc, level, (fl & 2) | 1)
        depth[i] = FR._norm(Pc[i])
    return track, depth


def frame_in_frustum_rig(P, cam, rig, points, bounds, nlevels):
    """Frame::isInFrustum, Nleft != -1 -> (left records, right records, mTrackDepth, mTrackDepthR, points either camera sees)"""
    tl, dl = _checks(P, cam, P["Tcw"], P["Ow"], points, bounds, nlevels)
    M, twc = rig_right_pose(P, rig)
    tr, dr = _checks(P, rig["cam2"], M, twc, points, bounds, nlevels)
    return tl, tr, dl, dr, int((((tl["flags"] | tr["flags"]) & 1) != 0).sum())
