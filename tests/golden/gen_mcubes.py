#!/usr/bin/env python3
"""Generate tests/golden/g18_mcubes.npz: marching-cubes inputs and scikit-image's meshes of them (numpy + scikit-image only;
run once wherever scikit-image is installed -- no test needs it).

    python tests/golden/gen_mcubes.py

    a  ellipsoid + sine, 48^3, level 0, spacing (0.05, 0.04, 0.03)      smooth: one vertex per crossing edge
    b  torus (axis z, centred; b.torus_R / b.torus_r) on a 40 x 48 x 36 grid, level 0.1, spacing 0.06   nx != ny != nz
    c  random normal 16^3 padded with a +1 border, level 0               ambiguous cells (only the input is compared)
Each holds {tag}.vol, .level, .spacing and scikit-image's {tag}.verts / .faces / .normals (Lewiner, defaults of the reference's
call: gradient_direction='descent', allow_degenerate=True), plus the scikit-image version string.
"""
import os

import numpy as np
import skimage
from skimage import measure

HERE = os.path.dirname(os.path.abspath(__file__))


def ellipsoid_sine(n=48):
    g = np.linspace(-1.0, 1.0, n)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    return (np.sqrt((x / 0.8) ** 2 + (y / 0.6) ** 2 + (z / 0.7) ** 2) - 1.0 + 0.05 * np.sin(6 * x) * np.cos(5 * y)).astype(np.float32)


TORUS = dict(R=0.65, r=0.35, s=0.06)       # level 0.1: tube radius 0.45 = 7.5 cells


def torus(shape=(40, 48, 36), R=TORUS["R"], r=TORUS["r"], s=TORUS["s"]):
    ax = [(np.arange(n) - (n - 1) / 2) * s for n in shape]
    x, y, z = np.meshgrid(*ax, indexing="ij")
    return (np.sqrt((np.sqrt(x ** 2 + y ** 2) - R) ** 2 + z ** 2) - r).astype(np.float32)


def random_padded(n=16, seed=0):
    v = np.random.default_rng(seed).standard_normal((n, n, n)).astype(np.float32)
    return np.pad(v, 1, constant_values=1.0)


def main():
    cases = {"a": (ellipsoid_sine(), 0.0, (0.05, 0.04, 0.03)), "b": (torus(), 0.1, (0.06, 0.06, 0.06)),
             "c": (random_padded(), 0.0, (1.0, 1.0, 1.0))}
    out = {"skimage_version": np.array(skimage.__version__), "b.torus_R": np.float64(TORUS["R"]), "b.torus_r": np.float64(TORUS["r"])}
    for tag, (vol, level, sp) in cases.items():
        verts, faces, normals, _ = measure.marching_cubes(vol, level, spacing=sp)
        out.update({f"{tag}.vol": vol, f"{tag}.level": np.float32(level), f"{tag}.spacing": np.array(sp, np.float32),
                    f"{tag}.verts": verts.astype(np.float32), f"{tag}.faces": faces.astype(np.int32),
                    f"{tag}.normals": normals.astype(np.float32)})
        print(f"{tag}: volume {vol.shape}, {len(verts)} vertices, {len(faces)} faces")
    path = os.path.join(HERE, "g18_mcubes.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}  {os.path.getsize(path) / 1024:.1f} KB (scikit-image {skimage.__version__})")


if __name__ == "__main__":
    main()
