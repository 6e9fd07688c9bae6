"""Generate tests/golden/g19_final_parsing.npz by running the REFERENCE's wireframe parsing (authoring container only).

    python tests/golden/make_parse_golden.py        # needs /root/reference ; writes tests/golden/g19_final_parsing.npz

The reference's code/neat-final-parsing.py is imported on the CPU with sys.modules stubs for GPUtil, pyhocon and trimesh (and for
imageio, skimage and cv2, which its utils import; none is called on this path) and Tensor.cuda = identity.  Its initial_recon and visibility_checking run with a stub model and loader that
return recorded per-chunk outputs of a synthetic wireframe scene: 6 views, about two thousand masked rays each, ground-truth lines with
noise and outliers, J = 64 junctions (20 near the scene's vertices).  The draw is repeated until every thresholded decision and every
argmin against its runner-up is more than 1e-4 relative away from flipping in float64 (tests/parse_f64.py), and until the reference's
Hungarian pairs equal scipy's on the float64 direct-difference cost matrix.  Only DATA is written.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/code"
sys.path.insert(0, REPO)

from tests import parse_f64 as F  # noqa: E402
from neat_amd.wireframe import WireframeGraph  # noqa: E402

N_VIEWS, J, RES, FOCAL, CHUNK = 6, 64, 512, 300.0, 2048
THR = dict(line_dis_threshold=10, line_score_threshold=0.01, junc_match_threshold=0.02, ckdist=100.0, ckview=5)
NAME_KWARGS = [
    {"conf": "../exps/abc-neat-a/00004926/2023_01_01_00_00_00/runconf.conf", "checkpoint": "latest", "distance": 10, "sdf_junction_refine": True},
    {"conf": "runconf.conf", "checkpoint": "1000", "distance": 10, "sdf_junction_refine": False},
    {"conf": "/data/exps/dtu/24/runconf.conf", "checkpoint": "latest", "distance": 5, "sdf_junction_refine": True},
    {"conf": "a/b/runconf.conf", "checkpoint": "2000", "distance": 20, "sdf_junction_refine": True},
]


def load_reference():
    for name in ("GPUtil", "trimesh", "imageio", "cv2", "skimage"):
        sys.modules[name] = types.ModuleType(name)
    ph = types.ModuleType("pyhocon")
    ph.ConfigFactory = type("ConfigFactory", (), {})
    sys.modules["pyhocon"] = ph
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    sys.path.insert(0, REF)
    spec = importlib.util.spec_from_file_location("neat_final_parsing", os.path.join(REF, "neat-final-parsing.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------ the synthetic scene
def look_at(centre):
    z = -centre / np.linalg.norm(centre)
    x = np.cross(np.array([0.0, 0.0, 1.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = R, -R @ centre
    return np.linalg.inv(w2c)


def sdf(x):
    return 0.01 * np.sin(3 * x[:, 0] + 1) * np.cos(2 * x[:, 1]) + 0.005 * x[:, 2]


def sdf_grad(x):
    return np.stack([0.03 * np.cos(3 * x[:, 0] + 1) * np.cos(2 * x[:, 1]), -0.02 * np.sin(3 * x[:, 0] + 1) * np.sin(2 * x[:, 1]),
                     np.full(len(x), 0.005)], -1)


def draw(seed):
    rng = np.random.default_rng(seed)
    verts = []
    while len(verts) < 20:
        p = rng.uniform(-0.6, 0.6, 3)
        if all(np.linalg.norm(p - q) > 0.25 for q in verts):
            verts.append(p)
    verts = np.array(verts)
    d = F.cdist(verts, verts)
    edges = set()
    for i in range(len(verts)):
        for j in np.argsort(d[i])[1:3]:
            edges.add((min(i, j), max(i, j)))
    segs = [(verts[i], verts[j]) for i, j in sorted(edges)]
    # a dangling line: one end a little past vertex A, the other 0.08 away where A is still the nearest junction -> edge (A, A)
    a = 0
    dirn = rng.normal(size=3)
    dirn /= np.linalg.norm(dirn)
    segs.append((verts[a] - 0.012 * dirn, verts[a] + 0.08 * dirn))
    junc = list(verts + rng.normal(0, 0.003, verts.shape))
    while len(junc) < J:
        p = rng.uniform(-1, 1, 3)
        if F.cdist(p[None], verts).min() > 0.15 and np.linalg.norm(p - segs[-1][1]) > 0.15:
            junc.append(p)
    junc = np.array(junc)[rng.permutation(J)]
    views = []
    drop = {e: rng.choice(N_VIEWS, size=rng.choice([0, 0, 1, 2]), replace=False) for e in range(len(segs))}
    # vertex 1 is not seen in view 0: its junction's first vote arrives later than those of junctions with higher indices
    for e, (i, j) in enumerate(sorted(edges)):
        if 1 in (i, j):
            drop[e] = np.union1d(drop[e][drop[e] != 0][:1], [0])
    for v in range(N_VIEWS):
        ang = 2 * np.pi * v / N_VIEWS + rng.uniform(-0.2, 0.2)
        pose = look_at(np.array([3 * np.cos(ang), 3 * np.sin(ang), rng.uniform(0.8, 1.6)]))
        K = np.array([[FOCAL, 0, RES / 2, 0], [0, FOCAL, RES / 2, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
        vertices, wedges, weights = [], [], []
        rows = {"lines3d": [], "lines2d": [], "l3d": []}
        for e, (p, q) in enumerate(segs):
            if v in drop[e]:
                continue
            if rng.random() < 0.5:
                p, q = q, p
            uv = F.project(K, pose, np.stack([p, q]))[0]
            g = uv + rng.normal(0, 0.3, 4)
            vertices += [g[:2], g[2:]]
            wedges.append([len(vertices) - 2, len(vertices) - 1])
            weights.append(0.03 if rng.random() < 0.08 else 0.99)
            k = int(rng.integers(20, 40)) if e == len(segs) - 1 else int(rng.integers(50, 110))
            noisy = e == 1
            for _ in range(k):
                l3 = np.stack([p, q]) + rng.normal(0, 0.004, (2, 3))
                l2 = g + rng.normal(0, 0.5, 4)
                t = rng.uniform()
                pt = p + t * (q - p) + rng.normal(0, 0.05 if noisy else 0.002, 3)
                if rng.random() < 0.5:
                    l3, l2 = l3[[1, 0]], l2[[2, 3, 0, 1]]
                rows["lines3d"].append(l3)
                rows["lines2d"].append(l2)
                rows["l3d"].append(pt)
        for _ in range(4):          # outlier ground-truth lines
            g = rng.uniform(0, RES, 4)
            vertices += [g[:2], g[2:]]
            wedges.append([len(vertices) - 2, len(vertices) - 1])
            weights.append(0.5)
        for _ in range(150):        # outlier rows
            rows["lines3d"].append(rng.uniform(-1, 1, (2, 3)))
            rows["lines2d"].append(rng.uniform(0, RES, 4))
            rows["l3d"].append(rng.uniform(-1, 1, 3))
        n = len(rows["l3d"])
        perm = rng.permutation(n)
        out = {k: np.array(x, np.float32)[perm] for k, x in rows.items()}
        out["lines2d"][rng.choice(n, 3, replace=False)] = np.nan
        wf = WireframeGraph(torch.tensor(np.array(vertices), dtype=torch.float32), torch.ones(len(vertices)),
                            torch.tensor(wedges, dtype=torch.long), torch.tensor(weights, dtype=torch.float32), RES, RES)
        out.update(K=K.astype(np.float32), pose=pose.astype(np.float32), wf=wf,
                   gt_lines_001=wf.line_segments(0.01).numpy(), gt_lines_005=wf.line_segments(0.05).numpy())
        views.append(out)
    return junc.astype(np.float32), views


class StubNet:
    def get_outputs(self, x):
        xn = x.double().numpy()
        return (torch.tensor(sdf(xn)[:, None], dtype=torch.float32), None, torch.tensor(sdf_grad(xn), dtype=torch.float32))

    def get_sdf_vals(self, x):
        return torch.tensor(sdf(x.double().numpy())[:, None], dtype=torch.float32)


class StubModel:
    """Returns the recorded per-chunk outputs of the view named by the input (split_input copies the dict, `view` included)."""

    def __init__(self, junc, views):
        self.views, self.off = views, {}
        self.latents = torch.tensor(junc)
        self.ffn = lambda latents: latents.clone()
        self.implicit_network = StubNet()

    def eval(self):
        return self

    def __call__(self, s):
        v, n = s["view"], s["uv"].shape[1]
        o = self.off.get(v, 0)
        self.off[v] = o + n
        vw = self.views[v]
        return {"lines3d": torch.tensor(vw["lines3d"][o:o + n]), "lines2d": torch.tensor(vw["lines2d"][o:o + n]).reshape(-1, 2, 2),
                "l3d": torch.tensor(vw["l3d"][o:o + n])}

    def project2D(self, K, R, T, X):
        from neat_amd.networks import VolSDFNetwork
        return VolSDFNetwork.project2D(None, K, R, T, X)


def loader(views):
    items = []
    for v, vw in enumerate(views):
        n = len(vw["l3d"])
        hw = n + 37
        mask = torch.zeros(1, hw, dtype=torch.bool)
        mask[0, torch.randperm(hw, generator=torch.Generator().manual_seed(v))[:n]] = True
        inp = {"mask": mask, "uv": torch.zeros(1, hw, 2), "uv_proj": torch.zeros(1, hw, 2), "lines": torch.zeros(1, hw, 5),
               "labels": torch.zeros(1, hw, dtype=torch.long), "intrinsics": torch.tensor(vw["K"])[None], "pose": torch.tensor(vw["pose"])[None],
               "wireframe": [vw["wf"]], "view": v}
        items.append((torch.tensor([v]), inp, {}))
    return items


def refined(junc, refine):
    g = torch.tensor(junc)
    if not refine:
        return g.numpy()
    net = StubNet()
    s, _, gr = net.get_outputs(g)
    g = g - s * gr
    return g[torch.argsort(net.get_sdf_vals(g).flatten())].numpy()


def run(mod, junc, views, refine):
    pairs = []
    inner = mod.linear_sum_assignment

    def recording(c):
        r = inner(c)
        pairs.append(r)
        return r
    mod.linear_sum_assignment = recording
    model = StubModel(junc, views)
    res = mod.initial_recon(model, loader(views), CHUNK, line_dis_threshold=THR["line_dis_threshold"],
                            junc_match_threshold=THR["junc_match_threshold"], sdf_junction_refine=refine)
    res["lines3d_wfi_checked"] = mod.visibility_checking(res["lines3d_wfi"], loader(views), model, mindis_th=THR["ckdist"],
                                                         min_visible_views=THR["ckview"], device="cpu")
    mod.linear_sum_assignment = inner
    return res, pairs


def main():
    mod = load_reference()
    for seed in range(100):
        junc, views = draw(seed)
        ok, out = True, {}
        for refine in (1, 0):
            res, pairs = run(mod, junc, views, bool(refine))
            jr = refined(junc, refine)
            f = F.distil(jr, views, **THR)
            ref_pairs = [p for p in f["pairs"] if p is not None]
            same_pairs = len(ref_pairs) == len(pairs) and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
                                                              for a, b in zip(ref_pairs, pairs))
            same = (same_pairs and np.array_equal(res["graph_initial"].numpy(), f["graph_initial"])
                    and res["lines3d_all"].shape[0] == f["lines3d_all"].shape[0]
                    and res["lines3d_wfi_checked"].shape[0] == f["lines3d_wfi_checked"].shape[0])
            diag = any(i == j for i, j in f["edges"])
            print(f"seed {seed} refine {refine}: margin {f['margin']:.2e}, same {same}, K {len(f['order'])}, N {len(f['lines3d_all'])}, "
                  f"E {len(f['edges'])}, checked {len(f['lines3d_wfi_checked'])}, diagonal {diag}")
            if not (f["margin"] > 1e-4 and same and diag and 0 < len(f["lines3d_wfi_checked"]) < len(f["edges"])
                    and f["order"] != sorted(f["order"])):
                ok = False
                break
            out[f"junctions_refine{refine}"] = jr.astype(np.float32)
            for k in ("junctions3d_initial", "lines3d_all", "graph_initial", "lines3d_wfi", "lines3d_wfi_checked"):
                out[f"r{refine}_{k}"] = res[k].numpy().astype(np.float32)
        if ok:
            break
    else:
        raise SystemExit("no draw with the required margins")
    out["junctions_raw"] = junc
    for v, vw in enumerate(views):
        for k in ("lines3d", "lines2d", "l3d", "gt_lines_001", "gt_lines_005", "K", "pose"):
            out[f"v{v}_{k}"] = np.asarray(vw[k], np.float32)
    out["n_views"] = np.array(N_VIEWS)
    out["seed"] = np.array(seed)
    names = [mod.make_hash_sha256(kw)[:8].replace("/", "n") for kw in NAME_KWARGS]
    out["name_kwargs"] = np.array(json.dumps(NAME_KWARGS))
    out["name_hashes"] = np.array(names)
    path = os.path.join(HERE, "g19_final_parsing.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, seed {seed}")


if __name__ == "__main__":
    main()
