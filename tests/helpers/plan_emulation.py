"""An independent NumPy statement of the frame plan's certificate (csrc/unwarp_kernels.hip plan_table_kernel, csrc/dcp_device.h
radial_rows_interp), for tests that must know how many wave tiles a plan OUGHT to certify before they look at what it reports.

Plain float64, no fused multiply-add anywhere: the radial factor f = E(r2) + ru O(r2) (even / odd Horner, as poly_inline orders it)
on every row of a 64 x 16 wave tile; the Newton cubic through rows 0, 5, 10, 15 as radial_rows_interp writes it
(f_k = f0 + k (d1 + (k - 5) (d2 + (k - 10) d3)), d1 = e1 * 0.2, d2 = s2 * 0.02, d3 = s3 * (1 / 750)); f xu + xc and f yu + yc rounded
to float32 both ways; a wave tile counts as reproduced when all 2 048 pairs have the same bit patterns.

What it leaves out on purpose -- the device's fused multiply-adds, and the tiles the device refuses because their box is clipped, does
not fit the slab or is not whole -- is what the factor one half in the tests' floor is for.  Wave tiles cut by the frame's right or
bottom edge count as not reproduced here, as on the device.
"""
import numpy as np

TILE_W, TILE_H = 64, 16
TINY_R2 = 1e-300


def radial_factor(r2, fact):
    """f(r2) with ru = sqrt(r2): E = a0 + r2 (a2 + ..), O = a1 + r2 (a3 + ..), f = ru O + E -- two roundings per step."""
    a = [float(v) for v in fact]
    nf = len(a)
    if nf == 0:
        return np.zeros_like(r2)
    ne, no = (nf + 1) // 2, nf // 2
    E = np.full_like(r2, a[2 * (ne - 1)])
    for k in range(ne - 2, -1, -1):
        E = r2 * E + a[2 * k]
    if no == 0:
        return E
    O = np.full_like(r2, a[2 * (no - 1) + 1])
    for k in range(no - 2, -1, -1):
        O = r2 * O + a[2 * k + 1]
    return np.sqrt(r2) * O + E


def emulated_certificate(shape, xc, yc, fact, y_origin=0):
    """(wave tiles, wave tiles whose interpolated rows reproduce the exact float32 coordinates) of an H x W frame; the first figure
    counts as the device does, four per 128 x 32 workgroup tile."""
    H, W = (int(v) for v in shape)
    xc, yc = float(xc), float(yc)
    whole_x = W // TILE_W
    xu = np.arange(whole_x * TILE_W, dtype=np.float64) - xc
    xx = xu * xu
    reproduced = 0
    for ty in range(H // TILE_H):
        yu = (np.arange(TILE_H, dtype=np.float64) + float(y_origin + ty * TILE_H)) - yc
        yy = np.maximum(yu * yu, TINY_R2)
        f = radial_factor(xx[None, :] + yy[:, None], fact)                   # (16, W'), exact on every row
        e1, e2, e3 = f[5] - f[0], f[10] - f[5], f[15] - f[10]
        s2, t2 = e2 - e1, e3 - e2
        s3 = t2 - s2
        d1, d2, d3 = e1 * 0.2, s2 * 0.02, s3 * (1.0 / 750.0)
        fi = f.copy()
        for k in range(1, 15):
            if k % 5:
                fi[k] = f[0] + float(k) * (d1 + float(k - 5) * (d2 + float(k - 10) * d3))
        xe, xi = (f * xu[None, :] + xc).astype(np.float32), (fi * xu[None, :] + xc).astype(np.float32)
        ye, yi = (f * yu[:, None] + yc).astype(np.float32), (fi * yu[:, None] + yc).astype(np.float32)
        same = (xe.view(np.uint32) == xi.view(np.uint32)) & (ye.view(np.uint32) == yi.view(np.uint32))
        reproduced += int(same.all(axis=0).reshape(whole_x, TILE_W).all(axis=1).sum())
    return 4 * (-(-W // 128)) * (-(-H // 32)), reproduced
