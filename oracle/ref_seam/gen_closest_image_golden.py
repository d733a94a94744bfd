"""Record what the reference's compiled Domain::closest_image returns (TEST INFRASTRUCTURE).

Runs oracle/_ref/ref_closest_image (the reference's own domain.cpp behind oracle/ref_seam/domain_harness.cpp, built by
`make -C oracle ref`) on the boxes and pairs constructed below and writes inputs and outputs, as float64, bit for bit:

    tests/golden/ref_closest_image.npz
        the boxes:       box_name, box_prd, box_tilt, box_periodic, box_triclinic; pairs first[b] .. first[b + 1] belong to
                         box b: xi, xj, xjimage [npairs, 3], klass [npairs]
        two 90-atom systems in tilted 16 A cells: sys_name, sys_prd, sys_tilt, sys_x [2, n, 3], sys_xjimage [2, n, n, 3]
                         (row i, column j = closest_image(x_i, x_j); the diagonal is the coincident pair)

Pair classes (klass): 0 = (a) random pairs inside the cell, 1 = (b) unwrapped pairs (each atom shifted by up to +-3 whole
lattice vectors independently: the reference's `while` loops run several times), 2 = (c) constructed ties (a component of
xj - xi exactly 0, +-L/2 or +-L, before or after the wraps of the other dimensions), 3 = (d) coincident points.
Classes (a) and (b) are all pairs between two small sets of points: the inputs then repeat, which is what keeps the
compressed file small.  Boxes in which ties are constructed have dyadic lengths and tilts, so every tie is exact.

    python oracle/ref_seam/gen_closest_image_golden.py          # rewrites the fixtures (same bytes every time)
"""
import io
import os
import subprocess
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
EXE = os.path.join(ROOT, "oracle", "_ref", "ref_closest_image")
GOLD = os.path.join(ROOT, "tests", "golden")

# name, prd, tilt (xy, xz, yz), periodic, triclinic
BOXES = [
    ("ortho_cubic", (16.0, 16.0, 16.0), (0.0, 0.0, 0.0), (1, 1, 1), 0),
    ("ortho_noncubic", (20.0, 14.0, 12.0), (0.0, 0.0, 0.0), (1, 1, 1), 0),
    ("tri_zero_tilt", (16.0, 16.0, 16.0), (0.0, 0.0, 0.0), (1, 1, 1), 1),
    ("tri_16_3p1", (16.0, 16.0, 16.0), (3.1, -2.2, 1.7), (1, 1, 1), 1),
    ("tri_16_half_pmp", (16.0, 16.0, 16.0), (8.0, -8.0, 8.0), (1, 1, 1), 1),
    ("tri_16_half_mpm", (16.0, 16.0, 16.0), (-8.0, 8.0, -8.0), (1, 1, 1), 1),
    ("tri_20_14_12_half", (20.0, 14.0, 12.0), (-10.0, 10.0, -7.0), (1, 1, 1), 1),
    ("tri_16_large_tilt", (16.0, 16.0, 16.0), (12.0, -4.0, 2.0), (1, 1, 1), 1),     # xy = 0.75 xprd: `box tilt large`
    ("ortho_ppf", (16.0, 16.0, 16.0), (0.0, 0.0, 0.0), (1, 1, 0), 0),
    ("tri_ppf", (16.0, 16.0, 16.0), (8.0, -8.0, 8.0), (1, 1, 0), 1),
    ("tri_fpp", (20.0, 14.0, 12.0), (-10.0, 10.0, -7.0), (0, 1, 1), 1),
]
SYSTEMS = [("t3p1", 16.0, (3.1, -2.2, 1.7), 101), ("t8", 16.0, (8.0, -8.0, 8.0), 102)]
NSYS, DMIN = 90, 1.9


def cell(prd, tilt):
    """rows a, b, c"""
    return np.array([[prd[0], 0.0, 0.0], [tilt[0], prd[1], 0.0], [tilt[1], tilt[2], prd[2]]])


def run_ref(prd, tilt, periodic, triclinic, xi, xj):
    xi, xj = np.ascontiguousarray(xi, np.float64), np.ascontiguousarray(xj, np.float64)
    head = np.array(list(prd) + list(tilt) + list(periodic) + [triclinic, len(xi)], np.float64)
    r = subprocess.run([EXE], input=head.tobytes() + np.hstack([xi, xj]).tobytes(), capture_output=True, check=True)
    return np.frombuffer(r.stdout, np.float64).reshape(len(xi), 3).copy()


def nearest_del(prd, tilt, periodic, d, reach=2):
    """brute force: the shortest of d + i a + j b + k c, |i|, |j|, |k| <= reach (periodic dimensions only)"""
    h = cell(prd, tilt)
    rng = [np.arange(-reach, reach + 1) if p else np.array([0]) for p in periodic]
    sh = np.array([i * h[0] + j * h[1] + k * h[2] for i in rng[0] for j in rng[1] for k in rng[2]])
    return np.sqrt(((d[:, None, :] + sh[None, :, :]) ** 2).sum(-1).min(-1))


def save_npz(path, **arrays):
    """np.savez_compressed with a fixed time stamp on every member: the same arrays give the same file"""
    with zipfile.ZipFile(path, "w") as z:
        for k, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def box_pairs(rng, prd, tilt, periodic, triclinic, dyadic):
    h = cell(prd, tilt)
    per = np.array(periodic, float)   # no lattice shifts along a non-periodic dimension
    xi, xj, kl = [], [], []
    # (a) all pairs between 18 and 15 random points of the cell
    pa, pb = rng.uniform(0, 1, (18, 3)) @ h, rng.uniform(0, 1, (15, 3)) @ h
    xi.append(np.repeat(pa, len(pb), 0)); xj.append(np.tile(pb, (len(pa), 1))); kl += [0] * (len(pa) * len(pb))
    # (b) the same with every point moved by up to +-3 lattice vectors of its own
    pa = rng.uniform(0, 1, (16, 3)) @ h + (rng.integers(-3, 4, (16, 3)) * per) @ h
    pb = rng.uniform(0, 1, (16, 3)) @ h + (rng.integers(-3, 4, (16, 3)) * per) @ h
    xi.append(np.repeat(pa, len(pb), 0)); xj.append(np.tile(pb, (len(pa), 1))); kl += [1] * (len(pa) * len(pb))
    # (c) ties.  xi on a 2^-10 grid; xj - xi = t + n . (a, b, c) with t_k in {0, +-L_k/2, +-L_k, one random grid value}:
    # in a dyadic box all of it is exact, the z wrap takes n_z c off and lands dy on t_y + n_y yprd, the y wrap lands dx on
    # t_x + n_x xprd.  In the one box with non-dyadic tilts only n = 0 is used (the ties are then in xj - xi itself).
    m = 90
    p = np.round(rng.uniform(0, 1, (m, 3)) * np.array(prd) * 1024) / 1024
    choice = rng.integers(0, 6, (m, 3))
    choice[:15] = np.array([[c0, c1, c2] for c0 in (1, 2) for c1 in (1, 2, 3) for c2 in (1, 2, 0)])[:15]  # all-tie rows
    tval = np.stack([np.zeros(3), 0.5 * np.array(prd), -0.5 * np.array(prd), np.array(prd), -np.array(prd)])
    t = np.where(choice < 5, tval[np.minimum(choice, 4), np.arange(3)[None, :]],
                 np.round(rng.uniform(-0.5, 0.5, (m, 3)) * np.array(prd) * 1024) / 1024)
    n = rng.integers(-2, 3, (m, 3)) * per if dyadic else np.zeros((m, 3))
    n[:30] = 0.0
    xi.append(p); xj.append(p + (t + n @ h)); kl += [2] * m
    # (d) coincident points, inside the cell and far outside
    p = rng.uniform(0, 1, (12, 3)) @ h
    p[6:] += (rng.integers(-3, 4, (6, 3)) * per) @ h
    xi.append(p); xj.append(p.copy()); kl += [3] * len(p)
    return np.vstack(xi), np.vstack(xj), np.array(kl, np.uint8)


def place_system(seed, L, tilt):
    """as tests/test_gpu_edges.py::test_triclinic_box_exact_mode: x = frac . (a, b, c), here with no two atoms (over all
    images) closer than DMIN"""
    rng = np.random.default_rng(seed)
    h = cell((L, L, L), tilt)
    sh = np.array([i * h[0] + j * h[1] + k * h[2] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)])
    x = np.zeros((0, 3))
    while len(x) < NSYS:
        p = rng.uniform(0, 1, 3) @ h
        if len(x) == 0 or np.sqrt((((x - p)[:, None, :] + sh[None]) ** 2).sum(-1)).min() >= DMIN:
            x = np.vstack([x, p])
    return x


def main():
    if not os.path.exists(EXE):
        sys.exit("build oracle/_ref/ref_closest_image first (make -C oracle ref)")
    rng = np.random.default_rng(20261018)
    XI, XJ, IM, KL, first = [], [], [], [], [0]
    for name, prd, tilt, periodic, tri in BOXES:
        dyadic = all(float(v * 4).is_integer() for v in tilt)
        xi, xj, kl = box_pairs(rng, prd, tilt, periodic, tri, dyadic)
        im = run_ref(prd, tilt, periodic, tri, xi, xj)
        ab = kl < 2
        far = np.sqrt(((im - xi) ** 2).sum(-1)) > nearest_del(prd, tilt, periodic, im - xi) * (1 + 1e-12) + 1e-12
        print("%-20s pairs %4d  not nearest (a, b): %3d = %.1f %%" % (name, len(xi), far[ab].sum(), 100.0 * far[ab].mean()))
        if tri and any(tilt):
            assert far[ab].sum() >= 20, name   # the condition the fixture has to meet, not a measurement
        XI.append(xi); XJ.append(xj); IM.append(im); KL.append(kl); first.append(first[-1] + len(xi))
    SX, SIM = [], []
    for name, L, tilt, seed in SYSTEMS:
        x = place_system(seed, L, tilt)
        i, j = np.divmod(np.arange(NSYS * NSYS), NSYS)
        im = run_ref((L, L, L), tilt, (1, 1, 1), 1, x[i], x[j]).reshape(NSYS, NSYS, 3)
        d = (im - x[:, None, :]).reshape(-1, 3)
        far = np.sqrt((d ** 2).sum(-1)) > nearest_del((L, L, L), tilt, (1, 1, 1), d) * (1 + 1e-12) + 1e-12
        print("system %-6s ordered pairs not nearest: %d of %d" % (name, far.sum(), NSYS * (NSYS - 1)))
        SX.append(x); SIM.append(im)
    out = os.path.join(GOLD, "ref_closest_image.npz")
    save_npz(
        out,
        box_name=np.array([b[0] for b in BOXES]), box_prd=np.array([b[1] for b in BOXES]),
        box_tilt=np.array([b[2] for b in BOXES]), box_periodic=np.array([b[3] for b in BOXES], np.int32),
        box_triclinic=np.array([b[4] for b in BOXES], np.int32), first=np.array(first, np.int64),
        xi=np.vstack(XI), xj=np.vstack(XJ), xjimage=np.vstack(IM), klass=np.concatenate(KL),
        sys_name=np.array([s[0] for s in SYSTEMS]), sys_prd=np.array([[s[1]] * 3 for s in SYSTEMS]),
        sys_tilt=np.array([s[2] for s in SYSTEMS]), sys_x=np.array(SX), sys_xjimage=np.array(SIM))
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
