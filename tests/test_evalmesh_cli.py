"""python -m neat_amd.mesh --eval on a run directory that holds a checkpoint of the synthetic geometric-initialisation model: the file
name, the bounding-box routes, the world transform, an existing file kept, and the PLY read back by neat_amd.evaluate."""
import os

import numpy as np
import pytest

from tests import evalmesh_f64 as E
from tests import mesh_f64 as M

pytestmark = pytest.mark.gpu
EPOCH = 7
BOX = np.array([[-0.5, -1.0, -1.0], [0.3, 1.0, 1.0]])      # what the pipeline uses; the npz holds its min row divided by 1.5


@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    from tests.util_run import write_synth_run
    run = write_synth_run(tmp_path_factory.mktemp("evalmesh_cli"), epoch=EPOCH, plot={"plot_nimgs": 1, "resolution": 100, "grid_boundary": [-1.5, 1.5]})["dir"]
    np.savez(run / "bbs.npz", **{"65": BOX / [[1.5], [1.0]]})
    S = np.eye(4)
    S[:3, :3] *= 300.0
    S[:3, 3] = [10.0, -20.0, 650.0]
    np.savez(run / "cameras.npz", scale_mat_0=S, world_mat_0=np.eye(4))
    return run


def cli(run, *args):
    from neat_amd import mesh
    assert mesh.main(["--conf", str(run / "runconf.conf"), "--eval", "--resolution", "40", "--precision", "fp32"] + [str(a) for a in args]) == 0


def test_eval_file_name_world_frame_and_kept_file(run_dir, capsys):
    from neat_amd import mesh, ply
    out = run_dir / str(EPOCH) / "scan.ply"
    cli(run_dir, "--no-world", "--cams", run_dir / "cameras.npz", "--normals")
    text = capsys.readouterr().out
    for stage in ("coarse", "frame", "fine grid", "extraction", "components"):
        assert stage in text
    assert str(out) == mesh.eval_out_path(str(run_dir), EPOCH) and out.exists()
    v, n, f = M.read_ply(str(out))
    assert n is not None and len(E.open_edges(f)) == 0 and np.abs(v).max() < 1.5      # the model's frame
    # kept unless --overwrite
    stamp = os.path.getmtime(out)
    cli(run_dir, "--cams", run_dir / "cameras.npz")
    assert "exists" in capsys.readouterr().out and os.path.getmtime(out) == stamp
    cli(run_dir, "--cams", run_dir / "cameras.npz", "--overwrite")
    w, wn, wf = M.read_ply(str(out))
    S = np.load(run_dir / "cameras.npz")["scale_mat_0"]
    assert wn is None and np.array_equal(wf, f) and np.array_equal(w, E.affine_rows(v, S[:3]))      # scale_mat_0 of --cams
    # the reader of the evaluation takes the file as it is
    back = ply.read_ply(str(out))
    assert np.array_equal(back["points"], w.astype(np.float64)) and np.array_equal(back["faces"], wf)


def test_bbox_file_with_its_quirk_equals_the_values_route(run_dir, capsys):
    out = run_dir / str(EPOCH) / "scan65.ply"
    cli(run_dir, "--bbox", run_dir / "bbs.npz", "--scan_id", "65")
    assert "cut" in capsys.readouterr().out and out.exists()
    first = out.read_bytes()
    v, _, f = M.read_ply(str(out))
    box = BOX.astype(np.float32)
    assert (v >= box[0]).all() and (v <= box[1]).all() and (v[:, 0] == box[1, 0]).any() and len(E.open_edges(f)) > 0
    cli(run_dir, "--scan_id", "65", "--overwrite", "--bbox-values", *[repr(float(x)) for x in BOX.reshape(-1)])
    assert out.read_bytes() == first
