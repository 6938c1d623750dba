"""numpy reference of the texture bake (include/ln3d_meshbake.h): the per-face atlas layout, the UV corners, the owner of every texel,
the point every owned texel maps to (float32, one rounding per operation, which is what the kernel promises) and the uint8 pack; and the
bilinear look-up a renderer does, with its taps laid open.  Written from the header's definition, texel by texel, not from mesh.py."""
import numpy as np

F32 = np.float32
LOWER = ((0.5, 0.5), (-2.5, 0.5), (0.5, -2.5))          # cell-local corners in texels; a negative entry e stands for c + e
UPPER = ((-0.5, -0.5), (2.5, -0.5), (-0.5, 2.5))


def layout(nf, size):
    """(n, c) or ValueError"""
    half = -(-nf // 2)
    n = 1
    while n * n < half:
        n += 1
    c = size // n
    if c < 4:
        raise ValueError(f"needs {4 * n}")
    return n, c


def uv_numerators(nf, size):
    """[nf,3,2] float64, exact: the corners in texel units (uv * size)"""
    n, c = layout(nf, size)
    out = np.zeros((nf, 3, 2))
    for f in range(nf):
        k = f // 2
        ox, oy = (k % n) * c, (k // n) * c
        for j, (a, b) in enumerate(UPPER if f % 2 else LOWER):
            out[f, j] = ox + (a if a > 0 else c + a), oy + (b if b > 0 else c + b)
    return out


def uvs(nf, size):
    return (uv_numerators(nf, size).astype(F32) / F32(size)).astype(F32)


def texels(nf, size):
    """owner [T*T] int32 (-1: nobody) and the cell-local coordinates a, b [T*T] of every texel (0 where it lies in the border strip)"""
    n, c = layout(nf, size)
    y, x = np.divmod(np.arange(size * size), size)
    inside = (x < n * c) & (y < n * c)
    a, b = np.where(inside, x % c, 0), np.where(inside, y % c, 0)
    f = 2 * ((y // c) * n + x // c) + (a + b > c - 1)
    owner = np.where(inside & (f < nf), f, -1).astype(np.int32)
    return owner, a, b


def points(verts, faces, size):
    """(points [T*T,3] float32, owner [T*T] int32)"""
    verts, faces = np.asarray(verts, F32), np.asarray(faces)
    n, c = layout(len(faces), size)
    owner, a, b = texels(len(faces), size)
    own = owner >= 0
    f = owner[own]
    upper = (f % 2 == 1)
    d = F32(c - 3)
    s = np.where(upper, c - 1 - a[own], a[own]).astype(F32) / d
    t = np.where(upper, c - 1 - b[own], b[own]).astype(F32) / d
    v0, v1, v2 = (verts[faces[f, j]] for j in range(3))
    out = np.zeros((size * size, 3), F32)
    out[own] = (v0 + s[:, None] * (v1 - v0)) + t[:, None] * (v2 - v0)              # float32 arrays: every operation rounds once
    assert out.dtype == F32
    return out, owner


def quantise(rgb):
    """the vertex-colour rule: clamp to [0, 1], times 255 in float32, truncate; NaN -> 0"""
    x = np.asarray(rgb, F32)
    with np.errstate(invalid='ignore'):
        y = np.where(np.isnan(x), F32(0), np.minimum(np.maximum(x, F32(0)), F32(1))).astype(F32)
    return np.trunc(y * F32(255)).astype(np.uint8)


def pack(rgb, owner, fill):
    out = quantise(rgb)
    out[np.asarray(owner) < 0] = fill
    return out


def taps(px, py, size):
    """the bilinear look-up at the texel-unit position (px, py) (float64; texel (x, y) has its centre at (x + 0.5, y + 0.5)): the list of
    (x, y, weight) with a NON-ZERO weight, indices clamped to the texture"""
    gx, gy = px - 0.5, py - 0.5
    x0, y0 = int(np.floor(gx)), int(np.floor(gy))
    fx, fy = gx - x0, gy - y0
    out = []
    for dx, wx in ((0, 1.0 - fx), (1, fx)):
        for dy, wy in ((0, 1.0 - fy), (1, fy)):
            if wx * wy != 0.0:
                out.append((min(max(x0 + dx, 0), size - 1), min(max(y0 + dy, 0), size - 1), wx * wy))
    return out


def lookup(tex, px, py):
    """tex [T,T,...] float64 sampled bilinearly at texel-unit positions px, py [N] -> [N,...]"""
    tex = np.asarray(tex, np.float64)
    out = np.zeros((len(px),) + tex.shape[2:])
    for i in range(len(px)):
        for x, y, w in taps(float(px[i]), float(py[i]), tex.shape[0]):
            out[i] += w * tex[y, x]
    return out


def bary_samples(rng, count):
    """[6 + count, 3] float64 barycentric weights: the corners, the edge midpoints and `count` random points; every weight is a multiple
    of 1 / 256 and they sum to 1 exactly, so a weighted sum of half-integer texel coordinates is exact in float64"""
    fixed = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, 0], [0, .5, .5], [.5, 0, .5]]
    i = rng.integers(0, 257, count)
    j = np.array([rng.integers(0, 257 - a) for a in i])
    return np.concatenate([np.array(fixed), np.stack([i, j, 256 - i - j], 1) / 256.0])


def soup(rng, nf, nv=None):
    """a random triangle soup inside the +-0.45 box: (verts [nv,3] float32, faces [nf,3] int64 with three distinct corners each)"""
    nv = nv or max(3, nf // 2 + 2)
    verts = rng.uniform(-0.45, 0.45, (nv, 3)).astype(F32)
    faces = np.stack([rng.permutation(nv)[:3] for _ in range(nf)]).astype(np.int64)
    return verts, faces
