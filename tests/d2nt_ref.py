"""numpy restatement of the D2NT "v3" depth-to-normal translator as the fine-tuning authors run it over Virtual KITTI 2
(depth-to-normal-translator/python/gen_vkitti_normals.py:100-133 around utils/myApis.py:48-179 and utils/apis.py:38-41), with the precision of every
step spelled out.  TEST INFRASTRUCTURE: the oracle of tests/test_d2nt_*.py and of scripts/d2nt_bench.py's host comparison; the product never imports it.

OpenCV's filter2D is restated as the stand-in that tests/golden/make_d2nt_golden.py runs the reference's own files over: correlation with
BORDER_REFLECT_101 (numpy's "reflect" pad), the result in the input dtype, fp32 accumulation over the kernel's NON-ZERO taps in row-major order."""
import numpy as np

E = np.e                            # myApis.py:84 base = np.e (a Python float: np.power(np.e, float32 array) stays float32 under numpy >= 2)
EPS = 1e-8                          # myApis.py:57, :110; apis.py:38
VKITTI_K = (725.0087, 725.0087, 620.5, 187.0)       # gen_vkitti_normals.py:70-73 (fx, fy, cx, cy; a float32 tensor there)
VKITTI_DEPTH_SCALE = 100.0                          # gen_vkitti_normals.py:107: metres back to centimetres, in float32


def _pad1(Z):
    return np.pad(Z, 1, mode="reflect")            # BORDER_REFLECT_101: Z[-1] = Z[1]


def gradients(Z):
    """myApis.py:86-89: grad_l/r/u/d = filter2D(Z, gradient_*) in fp32 (taps -1, +1 in row-major order: -Z[left] + Z[right])"""
    P = _pad1(Z)
    c = P[1:-1, 1:-1]
    gl = -P[1:-1, :-2] + c
    gr = -c + P[1:-1, 2:]
    gu = -P[:-2, 1:-1] + c
    gd = -c + P[2:, 1:-1]
    return gl, gr, gu, gd


def laplace_alpha(Z):
    """myApis.py:144: |filter2D(Z, [[0,-1,0],[-1,4,-1],[0,-1,0]])| in fp32, taps summed in row-major order"""
    P = _pad1(Z)
    c = P[1:-1, 1:-1]
    four = np.float32(4)
    return np.abs(((((-P[:-2, 1:-1]) + (-P[1:-1, :-2])) + four * c) + (-P[1:-1, 2:])) + (-P[2:, 1:-1]))


def soft_min(lap, direction, power=np.power):
    """myApis.py:48-70: fp32 powf, zero padding (not reflected) of the neighbour terms, fp64 from there on"""
    h, w = lap.shape
    p = power(E, -lap)
    assert p.dtype == np.float32
    if direction == 0:
        a = np.hstack([np.zeros((h, 1)), p[:, :-1]])
        b = np.hstack([p[:, 1:], np.zeros((h, 1))])
    else:
        a = np.vstack([np.zeros((1, w)), p[:-1, :]])
        b = np.vstack([p[1:, :], np.zeros((1, w))])
    return (a + EPS * 0.5) / (EPS + a + b), (b + EPS * 0.5) / (EPS + a + b)


def snap(la, lb, margins=None):
    """myApis.py:112-115 (and :117-120): four masked assignments in order, each testing the maps the previous lines modified.
    `margins` (list) collects |ratio / e - 1| of every test: how close the comparison came to flipping."""
    tests = ((0, 0, 1.0), (0, 1, 0.0), (1, 0, 0.0), (1, 1, 1.0))   # (ratio lb/la?, which map is assigned, value)
    m = [la, lb]
    for swap, dst, val in tests:
        r = (m[1] / (m[0] + EPS)) if swap else (m[0] / (m[1] + EPS))
        if margins is not None:
            margins.append(np.abs(r / E - 1.0))
        m[dst][r > E] = val
    return m[0], m[1]


def dag_gradients(Z, power=np.power, margins=None):
    """get_DAG_filter(Z) (myApis.py:84-125, lap_conf='1D-DLF'): the soft-min weighted one-sided gradients Gu, Gv in fp64"""
    gl, gr, gu, gd = gradients(Z)
    lap_hor, lap_ver = np.abs(gl - gr), np.abs(gu - gd)
    l1, l2 = soft_min(lap_hor, 0, power)
    l3, l4 = soft_min(lap_ver, 1, power)
    l1, l2 = snap(l1, l2, margins)
    l3, l4 = snap(l3, l4, margins)
    return l1 * gl + l2 * gr, l3 * gu + l4 * gd


def normals_v2(Z, K, power=np.power, margins=None):
    """gen_vkitti_normals.py:113-128: n = (Gu fx, Gv fy, -((Z + v Gv) + u Gu)) with 1-based pixel coordinates, divided by |n| + 1e-8 (fp64)"""
    fx, fy, cx, cy = (np.float32(k) for k in K)
    h, w = Z.shape
    u = np.ones((h, 1)) * np.arange(1, w + 1) - cx
    v = np.arange(1, h + 1).reshape(h, 1) * np.ones((1, w)) - cy
    Gu, Gv = dag_gradients(Z, power, margins)
    n = np.dstack((Gu * fx, Gv * fy, -(Z + v * Gv + u * Gu)))
    n /= (np.expand_dims(np.linalg.norm(n, axis=2), axis=2) + EPS)       # apis.py:38-41
    return n


def mrf_choice(Z):
    """MRF_optim's argmin (myApis.py:144-158, lap_conf='DLF-alpha'): 0 left, 1 right, 2 up, 3 down, 4 self; +inf outside the image"""
    h, w = Z.shape
    L = laplace_alpha(Z)
    inf = np.inf
    st = np.array((np.hstack((inf * np.ones((h, 1)), L[:, :-1])), np.hstack((L[:, 1:], inf * np.ones((h, 1)))),
                   np.vstack((inf * np.ones((1, w)), L[:-1, :])), np.vstack((L[1:, :], inf * np.ones((1, w)))), L))
    return np.argmin(st, axis=0)


def refine(n, choice):
    """MRF_optim's gather (myApis.py:159-178): each pixel takes the chosen neighbour's normal (zeros outside the image)"""
    h, w, _ = n.shape
    p = np.pad(n, ((1, 1), (1, 1), (0, 0)))
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    dy = np.array([0, 0, -1, 1, 0])[choice]
    dx = np.array([-1, 1, 0, 0, 0])[choice]
    return p[yy + 1 + dy, xx + 1 + dx]


def depth_to_normals(depth, K=VKITTI_K, refine_mrf=True, depth_scale=VKITTI_DEPTH_SCALE, power=np.power):
    """one image: depth fp32 [H,W] (metres for VKITTI) -> dict: normal fp64 [H,W,3] (after the final `* -1`, before quantisation), choice (MRF argmin,
    computed for v2 too), u16 (the file: ((n + 1) * 32767.5) truncated), u8 (what Image.open(p).convert('RGB') gives the loader: u16 >> 8),
    margin fp64 [H,W] (the smallest |ratio / e - 1| of the eight snapping tests of the pixel)"""
    Z = np.asarray(depth, dtype=np.float32) * np.float32(depth_scale)
    margins = []
    n = normals_v2(Z, K, power, margins)
    choice = mrf_choice(Z)
    if refine_mrf:
        n = refine(n, choice)
    n = n * -1
    u16 = ((n + 1) * 32767.5).astype(np.uint16)
    return {"normal": n, "choice": choice.astype(np.uint8), "u16": u16, "u8": (u16 >> 8).astype(np.uint8), "margin": np.min(np.stack(margins), axis=0)}


def correctly_rounded_power(base, x):
    """float32 base ** x rounded once from an fp64 exp: what csrc/d2nt.hip evaluates.  numpy's own float32 power is SIMD-dispatched (SVML on
    AVX-512 hosts) and differs from this by 1 ulp on a share of the inputs"""
    return np.exp(x.astype(np.float64) * np.log(np.float64(np.float32(base)))).astype(np.float32)


def vkitti_like_depth_cm(rng, H, W, sky=True):
    """seeded Virtual KITTI-like depth in integer centimetres (uint16): a ground plane whose depth grows towards the horizon, a sky at 65535 cm, fronto-
    parallel boxes (flat regions: exact argmin ties), a slanted wall, steps, and single-pixel spikes"""
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    hor = H * (0.3 + 0.2 * rng.random())
    d = np.where(yy > hor, 1.5 * 725.0 * 100.0 / np.maximum(yy - hor, 1e-3), 65535.0 if sky else 8000.0)
    for _ in range(max(1, (H * W) // 4000)):
        r = rng.random(6)
        x0, y0 = r[0] * W, hor * 0.5 + r[1] * (H - hor * 0.5)
        bw, bh = 2 + r[2] * W * 0.3, 2 + r[3] * H * 0.4
        box = (xx >= x0) & (xx < x0 + bw) & (yy >= y0 - bh) & (yy < y0)
        flat = 300 + r[4] * 4000
        d = np.where(box, flat + (r[5] > 0.6) * (xx - x0) * (3 + 40 * r[5]), d)
    wall = xx < W * 0.12 * rng.random()
    d = np.where(wall, 200 + 9.0 * xx + 0.5 * yy, d)
    d = np.where((yy.astype(int) % 17 == 5) & (xx < W / 2), d + 37, d)                  # steps
    band = (yy >= H * 0.55) & (yy < H * 0.55 + max(2, H // 8))                         # kinks of 1 cm / px: ratios at e within float32 round-off
    x1 = np.floor(W * (0.3 + 0.4 * rng.random()))
    d = np.where(band, 900 + np.maximum(0, xx - x1) + np.maximum(0, x1 - 5 - xx) * 2, d)
    spikes = rng.random((H, W)) < 0.002
    d = np.where(spikes, rng.integers(1, 65535, (H, W)), d)
    return np.clip(np.rint(d), 1, 65535).astype(np.uint16)


def cm_to_metres(cm):
    """VirtualKITTI2.__getitem__ (training/dataloaders/load.py:330, gen_vkitti_normals.py:63): uint16 centimetres -> float32 metres"""
    return cm.astype(np.float32) / 100.0
