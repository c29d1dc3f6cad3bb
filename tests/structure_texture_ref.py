"""numpy restatement of ofx_structure_texture_dev (include/ofx.h): the ROF structure part S of a frame by n_iter steps of Chambolle's
projection and the texture part T = f - alpha S (Wedel et al. 2009, section 3.1).  All arithmetic in float64, every operation
rounded once, association as written in the header; numpy's sqrt and / are correctly rounded.

Also what the tests around it share: the frames of every input kind, the illumination changes and the error measure of the
quality check."""
import functools

import numpy as np

IN_OPTION = {"u8": 1, "u16": 2, "f32": 3, "rgb8": 4}          # OFX_IN_*; the storage kinds are 0
THETA, ALPHA, N_ITER = 16.0, 0.95, 100                         # the header's recommendation for 8-bit frames


def divergence(p1, p2):
    """src/operators.cpp:36-78 with its border associations: the interior is (p1 - left) + (p2 - up); the first and last columns
    add p2 before they subtract the cell above"""
    ny, nx = p1.shape
    d = np.empty((ny, nx))
    d[1:-1, 1:-1] = (p1[1:-1, 1:-1] - p1[1:-1, :-2]) + (p2[1:-1, 1:-1] - p2[:-2, 1:-1])
    d[0, 1:-1] = (p1[0, 1:-1] - p1[0, :-2]) + p2[0, 1:-1]
    d[-1, 1:-1] = (p1[-1, 1:-1] - p1[-1, :-2]) - p2[-2, 1:-1]
    d[1:-1, 0] = (p1[1:-1, 0] + p2[1:-1, 0]) - p2[:-2, 0]
    d[1:-1, -1] = (-p1[1:-1, -2] + p2[1:-1, -1]) - p2[:-2, -1]
    d[0, 0] = p1[0, 0] + p2[0, 0]
    d[0, -1] = -p1[0, -2] + p2[0, -1]
    d[-1, 0] = p1[-1, 0] - p2[-2, 0]
    d[-1, -1] = -p1[-1, -2] - p2[-2, -1]
    return d


def forward_gradient(u):
    """src/operators.cpp:87-125: the difference to the right and downwards, 0 in the last column / row"""
    ux, uy = np.zeros(u.shape), np.zeros(u.shape)
    ux[:, :-1] = u[:, 1:] - u[:, :-1]
    uy[:-1, :] = u[1:, :] - u[:-1, :]
    return ux, uy


def decompose(f, theta=THETA, alpha=ALPHA, n_iter=N_ITER):
    """(S, T) in float64 of the frame's samples"""
    f = np.asarray(f, dtype=np.float64)
    r = 0.25 / theta
    p1, p2 = np.zeros(f.shape), np.zeros(f.shape)
    for _ in range(n_iter):
        u = f + theta * divergence(p1, p2)
        ux, uy = forward_gradient(u)
        g = 1.0 + r * np.sqrt(ux * ux + uy * uy)
        p1 = (p1 + r * ux) / g
        p2 = (p2 + r * uy) / g
    S = f + theta * divergence(p1, p2)
    return S, f - alpha * S


def texture(f, theta=THETA, alpha=ALPHA, n_iter=N_ITER):
    return decompose(f, theta, alpha, n_iter)[1]


def gray8(rgb):
    """the loader's rule for OFX_IN_RGB8: (uint8) (.299 R + .587 G + .114 B), products and sums rounded to double left to right"""
    c = rgb.astype(np.float64)
    return np.floor((.299 * c[..., 0] + .587 * c[..., 1]) + .114 * c[..., 2]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def frame(nx, ny, kind, seed=0):
    """a frame of the kind as the device reads it: (array to upload -- (ny, nx), rgb8: (ny, nx, 3) --, its samples in float64).
    Smooth shading, a step edge and noise, so that structure and texture are both there; read-only"""
    rng = np.random.default_rng(1000 * seed + 7 * nx + ny)
    i, j = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    base = 120.0 + 60.0 * np.sin(0.21 * j + 0.4 * seed) * np.cos(0.17 * i) + 40.0 * (j > 0.55 * nx) + rng.uniform(-25.0, 25.0, (ny, nx))
    if kind == "f64":
        a = base + rng.uniform(-0.5, 0.5, (ny, nx))
    elif kind == "f32":
        a = (base + rng.uniform(-0.5, 0.5, (ny, nx))).astype(np.float32)
    elif kind == "u8":
        a = np.clip(np.floor(base), 0, 255).astype(np.uint8)
    elif kind == "u16":
        a = np.clip(np.floor(base * 257.0), 0, 65535).astype(np.uint16)
    elif kind == "rgb8":
        a = np.clip(np.floor(base[..., None] + rng.uniform(-30.0, 30.0, (ny, nx, 3))), 0, 255).astype(np.uint8)
    else:
        raise ValueError(kind)
    a.setflags(write=False)
    vals = (gray8(a) if kind == "rgb8" else a).astype(np.float64)
    vals.setflags(write=False)
    return a, vals


def theta_for(kind):
    """theta = 16 * range / 255"""
    return THETA * 257.0 if kind == "u16" else THETA


@functools.lru_cache(maxsize=None)
def want(nx, ny, kind, n_iter, seed=0, alpha=ALPHA):
    """(S, T) in float64 for frame(nx, ny, kind, seed); read-only"""
    S, T = decompose(frame(nx, ny, kind, seed)[1], theta_for(kind), alpha, n_iter)
    S.setflags(write=False)
    T.setflags(write=False)
    return S, T


# ---- the quality check: illumination changes of the second frame, and the error against the synthetic truth ---------------------
def gain_ramp(I1):
    ny, nx = I1.shape
    j = np.arange(nx, dtype=np.float64)[None, :]
    return np.clip(np.floor(0.8 * I1 + 40.0 * j / nx + 10.0), 0, 255)


def shadow(I1):
    ny, nx = I1.shape
    i, j = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    return np.clip(np.floor(I1 * (1.0 - 0.35 * np.exp(-((j - 0.6 * nx) ** 2 + (i - 0.5 * ny) ** 2) / (2.0 * 30.0 ** 2)))), 0, 255)


CHANGES = {"unchanged": lambda I1: I1, "gain_ramp": gain_ramp, "shadow": shadow}


def mask(name, nx, ny):
    """8 px off every border; P1: also off the rectangle and where it moves to"""
    m = np.zeros((ny, nx), dtype=bool)
    m[8:ny - 8, 8:nx - 8] = True
    if name == "P1":
        m[ny // 4 - 6:ny // 2 + 6, nx // 4 - 2:nx // 2 + 10] = False
    return m


def aepe_truth(synth, name, u, v):
    ny, nx = u.shape
    i, j = synth._grid(nx, ny)
    tu, tv = synth._flow(i, j)
    m = mask(name, nx, ny)
    return float(np.mean(np.hypot(u - tu, v - tv)[m]))


def quality_pair(synth, name, change, nx=160, ny=120):
    """(I0, changed I1) of the pair"""
    I0, I1 = synth.pair(name, nx, ny)
    return I0, CHANGES[change](I1)
