"""The committed cases of the pixel selector: the smallest shapes at which each piece of it can go wrong.  Images are built from fixed
seeds with numpy alone; densities are literals chosen, on the CPU, so that each case takes the branch its name says and no comparison
is decided within 4 ulps (tests/test_select_oracle.py asserts both)."""
import ctypes
from types import SimpleNamespace

import numpy as np


def texture(H, W, seed, amp=60.0):
    """a smooth random texture on the 0 .. 255 scale, quantised to 1 / 8 so that sums and differences of neighbours are exact"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.full((H, W), 128.0)
    for _ in range(12):
        fx, fy = rng.uniform(-0.9, 0.9, 2)
        img += amp / 4 * rng.uniform(0.3, 1.0) * np.sin(fx * x + fy * y + rng.uniform(0, 6.28))
    img += rng.normal(0, amp / 12, (H, W))
    return (np.round(np.clip(img, 0, 255) * 8) / 8).astype(np.float32)


def table(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, H * W, dtype=np.uint8)


def reference_table(n):
    """what the reference's constructor draws: srand(3141592), rand() & 0xFF — the C library's generator, as
    eds_sel_fill_reference_pattern uses it"""
    libc = ctypes.CDLL(None)
    libc.srand(3141592)
    return np.array([libc.rand() & 0xFF for _ in range(n)], np.uint8)


def gamma_table():
    """a non-trivial CalibHessian::B: a monotone response with a varying slope"""
    i = np.arange(256, dtype=np.float64)
    return (255.0 * (i / 255.0) ** 1.6 + 0.25 * i).astype(np.float32)


def h_ramp(H, W, slope=2.5):
    """colour = slope * x: the gradient (slope, 0) is exactly orthogonal to direction 0 = (0, 1)"""
    return np.tile(np.arange(W, dtype=np.float32) * np.float32(slope), (H, 1))


def v_ramp(H, W, slope=2.5):
    """colour = slope * y: the gradient (0, slope) is exactly orthogonal to direction 14 = (1, 0)"""
    return np.tile((np.arange(H, dtype=np.float32) * np.float32(slope))[:, None], (1, W))


def sensitive_table(H, W, seed, nibble, first=0):
    """a table in which no entry before `first` draws direction `nibble` and a third of those from `first` on do.  Where EVERY cell is
    orthogonal to that direction, n2 stops for good at the first such entry: nothing after it can select"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, H * W, dtype=np.uint8)
    same = (t & 0xF) == nibble
    t[same] = (t[same] & 0xF0) | ((nibble + 3) & 0xF)
    hit = rng.random(H * W) < 1 / 3
    hit[:first] = False
    hit[first] = True
    t[hit] = (t[hit] & 0xF0) | nibble
    return t


def piecewise(H, W):
    """a continuous piecewise-linear image g(x + y) + 1.5 (x - y): diagonal stripes 8 wide with a constant gradient each — shallow,
    shallow, medium, shallow, shallow, steep — so dirNorm ties over whole stripes, and the first tied pixel of a 2 pot block in visiting
    order is not the first in raster order where a stripe enters the block through its second cell"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    slopes = np.array([1.0, 1.0, 5.0, 1.0, 1.0, 9.0])
    t = np.arange(H + W + 1)
    g = np.concatenate([[0.0], np.cumsum(slopes[(t[:-1] // 8) % 6])])
    return (g[(x + y).astype(int)] + 1.5 * (x - y) + 200.0).astype(np.float32)


def corner(H, W, seed):
    """texture in the top-left corner fading out, flat elsewhere"""
    t = texture(H, W, seed, amp=90.0).astype(np.float64) - 128.0
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    fade = np.clip(1.2 - np.hypot(x / (0.6 * W), y / (0.6 * H)), 0, 1) ** 2
    return (np.round((128.0 + t * fade) * 8) / 8).astype(np.float32)


def _case(name, image, tab, density, potential=3, recursions=1, th_factor=1.0, B=None, **prm):
    H, W = image.shape
    return SimpleNamespace(name=name, H=H, W=W, image=np.ascontiguousarray(image, np.float32), table=np.ascontiguousarray(tab, np.uint8),
                           density=float(density), potential=int(potential), recursions=int(recursions), th_factor=float(th_factor), B=B, prm=prm)


_cache = None


def cases():
    global _cache
    if _cache is not None:
        return _cache
    c = {}

    def add(*a, **k):
        x = _case(*a, **k)
        c[x.name] = x

    add("tex_64x96_sub", texture(64, 96, 11), table(64, 96, 1), density=70, potential=3, recursions=1)                # 0.25 <= quotia < 0.95
    add("tex_96x64_keep_th2_B", texture(96, 64, 32), table(96, 64, 2), density=350, potential=2, recursions=0, th_factor=2.0, B=gamma_table())
    add("odd_70x100_p1_ref", texture(100, 70, 13), reference_table(70 * 100), density=150, potential=1, recursions=2)   # recursion to a larger potential
    add("odd_70x100_p5_more", texture(100, 70, 14), table(100, 70, 4), density=600, potential=5, recursions=2)         # recursion to a smaller one
    add("odd_70x100_p40", texture(100, 70, 25), table(100, 70, 5), density=6, potential=40, recursions=0)             # one block larger than the image
    add("tex_64x96_nodist", texture(64, 96, 16), table(64, 96, 6), density=100, potential=2, recursions=1, select_direction_distribution=0)
    add("h_ramp_all_sensitive", h_ramp(64, 96), sensitive_table(64, 96, 7, 0, first=150), density=100, potential=3, recursions=0, min_grad_hist_add=0.0)
    add("v_ramp_all_sensitive", v_ramp(96, 64), sensitive_table(96, 64, 8, 14, first=90), density=100, potential=2, recursions=0, min_grad_hist_add=0.0)
    half = texture(100, 70, 17)
    half[:, 35:] = h_ramp(100, 70, 9.5)[:, 35:]
    add("half_ramp_some_sensitive", half, sensitive_table(100, 70, 9, 0), density=200, potential=3, recursions=1, th_factor=0.5, min_grad_hist_add=0.0)
    add("piecewise_ties", piecewise(64, 96), table(64, 96, 10), density=60, potential=3, recursions=0)
    add("flat", np.full((64, 96), 77.0, np.float32), table(64, 96, 21), density=100, potential=3, recursions=2)
    add("corner_levels", corner(96, 64, 18), table(96, 64, 22), density=40, potential=5, recursions=1)
    _cache = c
    return c
