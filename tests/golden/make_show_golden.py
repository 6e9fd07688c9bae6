"""Generate tests/golden/g21_show_cameras.npz from the REFERENCE's viewer (authoring container only).

    python tests/golden/make_show_golden.py        # needs /root/reference ; writes tests/golden/g21_show_cameras.npz

The reference's code/visualization/show.py is imported with sys.modules stubs for open3d, cv2, trimesh, GPUtil, pyhocon, pandas, tqdm and
pyquaternion (and for what its utils import; none is called here).  Recorded: its pose_spherical for the three camera presets at theta
offsets 0, 5 and 355 degrees, and the 2-D projection of the twelve edges of a cube through the inverse of each of those, by the arithmetic
of show.py:313-317 (K @ (R @ x.T + T), then the division) with this project's intrinsics.  Only numbers are written.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/code"
sys.path.insert(0, REPO)

from neat_amd import show  # noqa: E402

PRESETS = {"dtu": (-155, 0, -25, 3), "scan": (0, 170, -45, 3), "none": (0, 0, 0, 3)}      # show.py:459-471
OFFSETS = (0, 5, 355)
WIDTH, HEIGHT, FOV = 96, 80, 60.0


class _Anything(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Anything(self.__name__ + "." + name)

    def __call__(self, *a, **k):
        return self


def load_reference():
    for name in ("open3d", "cv2", "trimesh", "GPUtil", "pyhocon", "pandas", "tqdm", "pyquaternion", "imageio", "skimage", "skimage.measure",
                 "plotly", "plotly.graph_objs", "plotly.offline", "plotly.subplots", "torchvision", "utils", "utils.general", "utils.plots",
                 "utils.rend_util"):
        sys.modules.setdefault(name, _Anything(name))
    spec = importlib.util.spec_from_file_location("reference_show", os.path.join(REF, "visualization", "show.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cube_edges(half=0.5):
    c = np.array([[x, y, z] for x in (-half, half) for y in (-half, half) for z in (-half, half)], dtype=np.float64)
    pairs = [(i, j) for i in range(8) for j in range(i + 1, 8) if np.sum(c[i] != c[j]) == 1]
    return np.stack([c[[i, j]] for i, j in pairs])          # [12,2,3]


def main():
    mod = load_reference()
    K = show.intrinsics(WIDTH, HEIGHT, FOV)
    lines = cube_edges()
    out = {"K": K, "lines3d": lines, "width": np.array(WIDTH), "height": np.array(HEIGHT), "fov": np.array(FOV), "offsets": np.array(OFFSETS),
           "preset_names": np.array(list(PRESETS))}
    for name, (rx, ry, rz, t) in PRESETS.items():
        out["pose_" + name] = np.array([rx, ry, rz, t], dtype=np.float64)
        for off in OFFSETS:
            c2w = np.asarray(mod.pose_spherical(rx, (ry + off) % 360, rz, t))
            assert c2w.dtype == np.float64 and c2w.shape == (4, 4)
            extrinsic = np.linalg.inv(c2w)                    # show.py:292-294
            R, T = extrinsic[:3, :3], extrinsic[:3, 3:]
            x = lines.reshape(-1, 3)                          # show.py:313-317
            x2d = K @ (R @ x.transpose() + T)
            x2d = x2d[:2] / x2d[2:]
            x2d = x2d.transpose()
            out["c2w_%s_%d" % (name, off)] = c2w
            out["lines2d_%s_%d" % (name, off)] = x2d.reshape(-1, 2, 2)
    path = os.path.join(HERE, "g21_show_cameras.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
