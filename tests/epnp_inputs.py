"""Seeded inputs for the EPnP shape tests (tests/test_gpu_epnp_shapes.py on the GPU, tests/test_epnp_inputs_host.py for
the conditions the inputs themselves must meet, which need no GPU): models of n points, two cameras, the golden poses
projected through them, and the oracle's answer on every case -- computed once per process and shared."""
import numpy as np

from oracle import epnp_ref as E
from spef_amd.spe.keypoints import KeyPoints

B = 64                                  # rows per case: the first 64 golden poses
SWEEP_N = (6, 7, 12, 16)                # (a): compared against the oracle, noise-free and at 1 px
KAT_MODELS = (5, 6, 16, 'cube')         # (b): noise-free, against the true pose
CAMERAS = ('speed', 'second')
NOISE_PX = (0.0, 1.0)
# Base seed of the 1 px noise. With it (by the oracle alone, on the CPU) each of the three beta approximations wins
# at least 5 % of the noisy sweep rows: 188 / 177 / 147 of 512; test_epnp_inputs_host.py keeps that true.
NOISE_SEED = 100


class Cam:
    def __init__(self, K, nu, nv, dist=None):
        self.K, self.nu, self.nv = np.asarray(K, np.float64), float(nu), float(nv)
        if dist is not None:
            self.distCoeffs = np.asarray(dist, np.float64)


def speed_camera(g):
    """The camera of tests/golden/keypoints.npz: square pixels, centred principal point, 1920 x 1200."""
    return Cam(g['K'], float(g['nu']), float(g['nv']))


def second_camera():
    """Non-square pixels, a principal point well off the image centre (640, 480), another image size."""
    return Cam([[1500.0, 0.0, 700.0], [0.0, 1250.0, 400.0], [0.0, 0.0, 1.0]], 1280.0, 960.0)


# t[:, :2] of the golden poses (SPEED frustum: |x / z| up to 0.32, |y / z| up to 0.2) times this keeps the object in
# the second camera's narrower side (580 / 1500 = 0.39 to the right of the principal point, 400 / 1250 = 0.32 above it)
SECOND_XY_SCALE = 0.8


def model(n):
    """n float32 points uniform in +-0.5 m (seed = n), or the 8 corners of a +-0.3 m cube: three equal PCA eigenvalues,
    so the control-point axes are arbitrary."""
    if n == 'cube':
        pts = np.array([[x, y, z] for x in (-0.3, 0.3) for y in (-0.3, 0.3) for z in (-0.3, 0.3)], np.float32)
    else:
        pts = np.random.default_rng(1000 + n).uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    assert np.linalg.svd(pts - pts.mean(0), compute_uv=False).min() > 0.05
    return np.ascontiguousarray(pts)


def poses(g, camera):
    q, t = g['q'][:B].astype(np.float64), g['t'][:B].astype(np.float64).copy()
    if camera == 'second':
        t[:, :2] *= SECOND_XY_SCALE
    return q, t


def camera_of(g, camera):
    return speed_camera(g) if camera == 'speed' else second_camera()


def project(cam, pts, q, t):
    kps = KeyPoints(cam, pts)
    return np.stack([kps.create_keypoints2d(q[i], t[i]) for i in range(q.shape[0])])


def add_noise(kp, cam, px, seed):
    if px == 0:
        return kp
    n1 = kp.shape[1] // 2
    rng = np.random.default_rng(seed)
    return (kp + rng.normal(0, px, kp.shape) / np.tile([cam.nu, cam.nv], n1)).astype(np.float32)


def in_frame_fraction(kp):
    return float(np.mean(np.all((kp[:, 2:] > 0) & (kp[:, 2:] < 1), axis=1)))


_cache = {}


def case(g, n, camera, px):
    """-> dict(pts, cam, kp [B x 2(n+1)] float32, q, t (truth), rq, rt, win (the oracle's), inside)."""
    key = (n, camera, px)
    if key not in _cache:
        cam, pts = camera_of(g, camera), model(n)
        q, t = poses(g, camera)
        clean = project(cam, pts, q, t)
        kp = add_noise(clean, cam, px, NOISE_SEED + (n if n != 'cube' else 8) + (50 if camera == 'second' else 0))
        rq, rt, win = E.decode_batch(kp, pts, cam.K, cam.nu, cam.nv, None, return_winner=True)
        _cache[key] = dict(pts=pts, cam=cam, kp=np.ascontiguousarray(kp), q=q, t=t, rq=rq, rt=rt, win=win,
                           inside=in_frame_fraction(clean))
    return _cache[key]


def noisy_sweep_winners(g):
    """The oracle's winning approximation of every noisy row of the sweep (a): 4 n x 2 cameras x 64 rows."""
    return np.concatenate([case(g, n, cam, 1.0)['win'] for n in SWEEP_N for cam in CAMERAS])


# ---- (e) distortion edges: the SPEED+ camera's K with other coefficient sets
# 1 + k1 r^2 + k2 r^4 + k3 r^6 < 0 from r^2 ~ 1 / |k1| = 0.083 outwards. The fixture's keypoints reach r^2 = 0.075 and
# undistortPoints' iteration x <- x0 / (1 + k1 r^2 ...) pushes the outer ones across, so the outermost keypoints of
# some rows take its icdist < 0 fallback while most points do not.
STRONG_K1 = -12.0
DIST_KINDS = ('4coef_mild', '4coef', '5coef')


def distortion_case(gp, kind):
    """gp = tests/golden/keypoints_speedplus.npz. '4coef_mild': its (k1, k2, p1, p2) without k3; '4coef' / '5coef':
    k1 = STRONG_K1 without / with k3. The pixels are the fixture's own projections of the first 64 poses with 1 px
    noise, the same for the GPU and the oracle (for the strong k1 they are no physical projection through that lens).
    -> dict(dist, cam, kp, rq, rt, fell [B x 11] bool: the oracle's undistort_points took the fallback)."""
    key = ('dist', kind)
    if key not in _cache:
        d = np.asarray(gp['dist'], np.float64).reshape(-1)
        dist = {'4coef_mild': d[:4].copy(), '4coef': np.array([STRONG_K1, d[1], d[2], d[3]]),
                '5coef': np.array([STRONG_K1, d[1], d[2], d[3], d[4]])}[kind]
        cam = Cam(gp['K'], float(gp['nu']), float(gp['nv']))
        kp = add_noise(gp['kp2d'][:B], cam, 1.0, 8)
        fell = np.stack([E.undistort_points(E.pixels_f32(kp[i], cam.nu, cam.nv), cam.K, dist, return_fallback=True)[1]
                         for i in range(B)])
        rq, rt = E.decode_batch(kp, gp['kp3d'], cam.K, cam.nu, cam.nv, dist)
        _cache[key] = dict(dist=dist, cam=cam, kp=np.ascontiguousarray(kp), rq=rq, rt=rt, fell=fell)
    return _cache[key]
