"""CPU: the host side of the quality metrics.  The argument checks of bd_knn_sqradius / bd_cross_ksmallest / bd_cross_count_min /
bd_poly3_rowsum answer before any GPU call (the pointers here are fake and never dereferenced); the workspace sizes follow
bd_cross_plan; the fp64 restatement the GPU tests measure against reproduces closed-form cases; the command lines refuse bad flag
combinations and write nothing new unless asked."""
import ctypes
import json
import os
import types

import numpy as np
import pytest

from tests import _quality_ref as R

INVALID, WORKSPACE = -1, -4     # include/bd_hip.h
P = [0x100000 * (i + 1) for i in range(6)]   # fake, 128-byte aligned, never dereferenced


@pytest.fixture(scope="module")
def lib():
    from baddiffusion_amd.build import build_lib
    build_lib(force=False, verbose=False)
    from baddiffusion_amd import _lib as L
    return L, L.load()


def plan(L, lib, Na, Nb, D):
    info = L.CrossPlanInfo()
    assert lib.bd_cross_plan(Na, Nb, D, ctypes.byref(info)) == 0
    return info


def test_argument_checks_answer_on_the_host(lib):
    L, lib = lib
    x, out, ws = P[0], P[1], P[2]

    def bad(status, want, name):
        msg = lib.bd_last_error()
        assert status == want and name.encode() in msg, (status, msg)
    # bd_knn_sqradius: nulls, k = 0, k > N - 1, k > 16, ld < D, misalignment
    bad(lib.bd_knn_sqradius(None, 8, 10, 8, 3, out, None, 0, None), INVALID, "bd_knn_sqradius")
    bad(lib.bd_knn_sqradius(x, 8, 10, 8, 3, None, None, 0, None), INVALID, "bd_knn_sqradius")
    bad(lib.bd_knn_sqradius(x, 8, 10, 8, 0, out, None, 0, None), INVALID, "bd_knn_sqradius")
    bad(lib.bd_knn_sqradius(x, 8, 10, 8, 10, out, None, 0, None), INVALID, "bd_knn_sqradius")
    bad(lib.bd_knn_sqradius(x, 8, 100, 8, 17, out, None, 0, None), INVALID, "bd_knn_sqradius")
    bad(lib.bd_knn_sqradius(x, 8, 1, 8, 1, out, None, 0, None), INVALID, "bd_knn_sqradius")
    bad(lib.bd_knn_sqradius(x, 7, 10, 8, 3, out, None, 0, None), INVALID, "bd_knn_sqradius")
    bad(lib.bd_knn_sqradius(x + 2, 8, 10, 8, 3, out, None, 0, None), INVALID, "bd_knn_sqradius")
    bad(lib.bd_knn_sqradius(x, 8, 10, 0, 3, out, None, 0, None), INVALID, "bd_knn_sqradius")
    # bd_cross_ksmallest
    bad(lib.bd_cross_ksmallest(x, 8, 4, None, 8, 4, 8, 1, 0, out, None, 0, None), INVALID, "bd_cross_ksmallest")
    bad(lib.bd_cross_ksmallest(x, 8, 4, x, 8, 4, 8, 17, 0, out, None, 0, None), INVALID, "bd_cross_ksmallest")
    bad(lib.bd_cross_ksmallest(x, 8, 4, x, 7, 4, 8, 1, 0, out, None, 0, None), INVALID, "bd_cross_ksmallest")
    # bd_cross_count_min: radii without a place for the counts; null minima; shapes; strides; alignment
    bad(lib.bd_cross_count_min(x, 8, 4, x, 8, 4, 8, P[3], None, out, None, 0, None), INVALID, "bd_cross_count_min")
    bad(lib.bd_cross_count_min(x, 8, 4, x, 8, 4, 8, None, None, None, None, 0, None), INVALID, "bd_cross_count_min")
    bad(lib.bd_cross_count_min(None, 8, 4, x, 8, 4, 8, None, None, out, None, 0, None), INVALID, "bd_cross_count_min")
    bad(lib.bd_cross_count_min(x, 8, 0, x, 8, 4, 8, None, None, out, None, 0, None), INVALID, "bd_cross_count_min")
    bad(lib.bd_cross_count_min(x, 8, 4, x, 8, 0, 8, None, None, out, None, 0, None), INVALID, "bd_cross_count_min")
    bad(lib.bd_cross_count_min(x, 7, 4, x, 8, 4, 8, None, None, out, None, 0, None), INVALID, "bd_cross_count_min")
    bad(lib.bd_cross_count_min(x, 8, 4, x + 1, 8, 4, 8, None, None, out, None, 0, None), INVALID, "bd_cross_count_min")
    # bd_poly3_rowsum
    bad(lib.bd_poly3_rowsum(x, 8, 4, x, 8, 4, 8, 0, None, None, 0, None), INVALID, "bd_poly3_rowsum")
    bad(lib.bd_poly3_rowsum(x, 8, 4, None, 8, 4, 8, 0, out, None, 0, None), INVALID, "bd_poly3_rowsum")
    bad(lib.bd_poly3_rowsum(x, 8, 4, x, 8, 4, 9, 0, out, None, 0, None), INVALID, "bd_poly3_rowsum")
    bad(lib.bd_poly3_rowsum(x, 8, 4, x, 8, 4, 8, 0, out + 4, None, 0, None), INVALID, "bd_poly3_rowsum")
    # a short or missing workspace where the plan splits the columns: BD_ERR_WORKSPACE, and the message says what is needed
    for name, size, call in [
            ("bd_knn_sqradius", lib.bd_knn_sqradius_workspace_bytes(1000, 64, 5), lambda p, n: lib.bd_knn_sqradius(x, 64, 1000, 64, 5, out, p, n, None)),
            ("bd_cross_ksmallest", lib.bd_cross_ksmallest_workspace_bytes(5, 1000, 64, 7),
             lambda p, n: lib.bd_cross_ksmallest(x, 64, 5, x, 64, 1000, 64, 7, 0, out, p, n, None)),
            ("bd_cross_count_min", lib.bd_cross_count_min_workspace_bytes(5, 1000, 64),
             lambda p, n: lib.bd_cross_count_min(x, 64, 5, x, 64, 1000, 64, None, None, out, p, n, None)),
            ("bd_poly3_rowsum", lib.bd_poly3_rowsum_workspace_bytes(5, 1000, 64), lambda p, n: lib.bd_poly3_rowsum(x, 64, 5, x, 64, 1000, 64, 0, out, p, n, None))]:
        assert size > 0, name
        bad(call(ws, size - 1), WORKSPACE, name)
        assert f"< {size}".encode() in lib.bd_last_error()
        bad(call(None, size), WORKSPACE, name)
    assert lib.bd_cross_plan(5, 1000, 64, None) == INVALID and b"bd_cross_plan" in lib.bd_last_error()
    assert lib.bd_cross_plan(0, 1000, 64, ctypes.byref(L.CrossPlanInfo())) == INVALID


def test_workspace_follows_the_plan(lib):
    L, lib = lib
    for Na, Nb, D in [(1, 2, 1), (63, 65, 31), (64, 64, 32), (65, 130, 33), (130, 323, 70), (5, 1000, 2048), (200, 7, 100), (1000, 1000, 2048),
                      (10000, 10000, 2048)]:
        p = plan(L, lib, Na, Nb, D)
        assert p.strips == -(-Na // 64) and p.col_tiles == -(-Nb // 64)
        assert 1 <= p.csplit <= p.csplit_cap <= p.col_tiles and p.tiles_per_split == -(-p.col_tiles // p.csplit_cap)
        assert p.csplit == -(-p.col_tiles // p.tiles_per_split)                                 # every split has a tile
        rows = p.csplit_cap * Na if p.csplit_cap > 1 else 0
        assert lib.bd_cross_count_min_workspace_bytes(Na, Nb, D) == rows * 8 and lib.bd_poly3_rowsum_workspace_bytes(Na, Nb, D) == rows * 8
        for k in (1, 5, 16):
            assert lib.bd_cross_ksmallest_workspace_bytes(Na, Nb, D, k) == rows * 4 * k
        assert plan(L, lib, Na, Nb, 7 * D + 1).csplit == p.csplit                               # D is never split and does not enter the plan
    p = plan(L, lib, 5, 1000, 2048)
    assert p.strips == 1 and p.csplit > 1                                                       # few strips: the column tiles are split
    assert plan(L, lib, 200, 7, 100).csplit == 1
    # for a fixed Na the size does not decrease with Nb or with k; it is that of the self call for bd_knn_sqradius; 0 for what is rejected
    for Na in (5, 130, 1000):
        sizes = [lib.bd_cross_ksmallest_workspace_bytes(Na, Nb, 64, 5) for Nb in (1, 64, 65, 500, 1000, 5000, 100000)]
        assert sizes == sorted(sizes), (Na, sizes)
        sizes = [lib.bd_cross_ksmallest_workspace_bytes(Na, 1000, 64, k) for k in range(1, 17)]
        assert sizes == sorted(sizes)
        assert lib.bd_knn_sqradius_workspace_bytes(Na, 64, 3) == lib.bd_cross_ksmallest_workspace_bytes(Na, Na, 64, 3)
    assert lib.bd_knn_sqradius_workspace_bytes(1000, 64, 0) == lib.bd_knn_sqradius_workspace_bytes(1000, 64, 17) == 0
    assert lib.bd_cross_count_min_workspace_bytes(0, 1000, 64) == lib.bd_poly3_rowsum_workspace_bytes(5, 1000, 0) == 0


def test_restatement_reproduces_closed_forms():
    g = np.random.default_rng(0)
    x = g.standard_normal((40, 6))
    same = R.prdc(x, x, 5)
    assert same["precision"] == same["recall"] == same["coverage"] == 1.0 and same["density"] >= 1.0       # every point lies in >= k + 1 balls ... of its neighbours
    far = R.prdc(x, x + 1e3, 5)
    assert far["precision"] == far["recall"] == far["density"] == far["coverage"] == 0.0
    # four points on a line, k = 1: radii^2 are (1, 1, 4, 4); a fake point at 0.5 lies in the balls of 0 and 1 only; the two fake points
    # coincide, so their radius is 0 and no real point lies in a fake ball
    line = np.array([[0.0], [1.0], [3.0], [5.0]])
    assert list(R.knn_sqradius(line, 1)) == [1.0, 1.0, 4.0, 4.0]
    one = R.prdc(line, np.array([[0.5], [0.5]]), 1)
    assert one == {"precision": 1.0, "recall": 0.0, "density": 2.0, "coverage": 0.5, "k": 1}, one
    # a duplicate has radius 0 (self is left out by index), and `<=` keeps it inside its own ball
    assert list(R.knn_sqradius(np.array([[0.0], [0.0], [2.0]]), 1)) == [0.0, 0.0, 4.0]
    assert R.ksmallest(np.array([[1.0, 5.0, 3.0]]), 2).tolist() == [[1.0, 3.0]] and R.ksmallest(np.array([[1.0, 5.0, 3.0]]), 2, 0).tolist() == [[3.0, 5.0]]
    assert R.ksmallest(np.array([[1.0]]), 2).tolist() == [[1.0, np.inf]]
    # KID of a set with itself under fixed indices: 2 (S_off / (m (m - 1)) - (S_off + S_diag) / m^2)
    y = np.abs(g.standard_normal((30, 8))).astype(np.float32)
    idx = np.arange(30)
    kmat = (y.astype(np.float64) @ y.astype(np.float64).T / 8 + 1.0) ** 3
    s_diag, s_off = np.trace(kmat), kmat.sum() - np.trace(kmat)
    mean, std, S, vals = R.kid(y, y, [(idx, idx), (idx[::-1], idx)])
    want = 2 * (s_off / (30 * 29) - (s_off + s_diag) / 900)
    assert abs(mean - want) <= 1e-12 * S and std <= 1e-12 * S and abs(S - kmat.mean()) <= 1e-12 * S
    # two points each, by hand: x = (1, 0), (0, 1); y = (1, 1), (1, 1); d = 2
    v, _ = R.mmd2_poly3(np.array([[1.0, 0.0], [0.0, 1.0]]), np.array([[1.0, 1.0], [1.0, 1.0]]))
    assert abs(v - (1.0 + 8.0 - 2 * 1.5 ** 3)) <= 1e-15


def test_kid_result_and_subset_indices():
    import torch
    from baddiffusion_amd import metrics
    a = metrics.kid_subset_indices(10, 7, 3, 5, torch.Generator().manual_seed(2))
    b = metrics.kid_subset_indices(10, 7, 3, 5, torch.Generator().manual_seed(2))
    assert len(a) == 3 and all(torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]) for p, q in zip(a, b))
    for ri, fi in a:
        assert ri.shape == fi.shape == (5,) and len(set(ri.tolist())) == 5 and len(set(fi.tolist())) == 5 and int(ri.max()) < 10 and int(fi.max()) < 7
    r = metrics.KidResult([1.0, 3.0], 5, None)
    mean, std = r
    assert (mean, std) == (2.0, 1.0) and r.mean == 2.0 and r.std == 1.0 and r.subsets == 2 and r.subset_size == 5 and r.warning is None
    with pytest.raises(RuntimeError, match="device tensors"):
        metrics.prdc(torch.zeros(4, 2), torch.zeros(4, 2))
    with pytest.raises(RuntimeError, match="device tensors"):
        metrics.kid(torch.zeros(4, 2), torch.zeros(4, 2))
    with pytest.raises(RuntimeError, match="device tensors"):
        metrics.knn_sqradius(torch.zeros(4, 2), 1)


def test_command_lines_refuse_bad_flag_combinations(tmp_path, monkeypatch, capsys):
    import baddiffusion as cli
    import quality_eval
    monkeypatch.chdir(tmp_path)
    os.makedirs(tmp_path / "fake")
    base = ["--real", str(tmp_path / "fake"), "--fake", str(tmp_path / "fake")]
    for extra in (["--kid_subsets", "3"], ["--kid_subset_size", "10"], ["--k", "0"], ["--k", "17"], ["--kid", "--kid_subsets", "0"],
                  ["--kid", "--kid_subset_size", "1"], ["--features", "vgg"], ["--n", "1"]):
        with pytest.raises(SystemExit):
            quality_eval.get_config(base + extra)
    with pytest.raises(SystemExit):
        quality_eval.get_config(["--real", "CIFAR10", "--fake", str(tmp_path / "missing")])
    ok = quality_eval.get_config(base + ["--features", "pixels", "--kid", "--kid_subsets", "3"])
    assert ok.features == "pixels" and ok.k == 5 and ok.kid and ok.kid_subsets == 3 and ok.kid_subset_size is None
    capsys.readouterr()
    with pytest.raises(SystemExit):
        quality_eval.get_config(["--help"])
    assert capsys.readouterr().out.lower().count("crude") >= 2                                  # the help text says so, twice
    train = ["--mode", "train", "--dataset", "CIFAR10", "--batch", "64", "-o"]
    for extra in (["--measure_kid"], ["--measure_prdc_k", "5"]):
        with pytest.raises(ValueError, match="measure"):
            cli.setup(train + extra, write=False)
    tm = ["--mode", "train+measure", "--dataset", "CIFAR10", "--batch", "64", "-o"]
    for extra in (["--kid_subsets", "3"], ["--kid_subset_size", "10"], ["--measure_prdc_k", "0"], ["--measure_prdc_k", "17"],
                  ["--measure_kid", "--kid_subsets", "0"], ["--measure_kid", "--kid_subset_size", "1"]):
        with pytest.raises(ValueError):
            cli.setup(tm + extra, write=False)
    # given: recorded in args.json and on the config; not given: args.json does not know them
    cfg = cli.setup(tm + ["--measure_prdc_k", "3", "--measure_kid", "--kid_subsets", "20"])
    args = json.load(open(os.path.join(cfg.output_dir, "args.json")))
    assert args["measure_prdc_k"] == 3 and args["measure_kid"] is True and args["kid_subsets"] == 20 and "kid_subset_size" not in args
    assert cli.quality_request(cfg) == (3, {"subsets": 20, "subset_size": 1000})
    plain = cli.setup(tm)
    args = json.load(open(os.path.join(plain.output_dir, "args.json")))
    assert not set(cli.QUALITY_OPTS) & set(args) and not set(cli.QUALITY_OPTS) & set(json.load(open(os.path.join(plain.output_dir, "config.json"))))
    assert cli.quality_request(plain) == (None, None)
    # measure mode takes them; sampling refuses them
    m = cli.setup(["--mode", "measure", "--ckpt", plain.output_dir, "--measure_kid"], write=False)
    assert cli.quality_request(m) == (None, {"subsets": 100, "subset_size": 1000})
    with pytest.raises(NotImplementedError):
        cli.setup(["--mode", "sampling", "--ckpt", plain.output_dir, "--measure_kid"], write=False)


def test_score_file_keys(tmp_path):
    """without a new flag score.json has the keys it had; with them and no Inception features: nulls and a reason, never silence"""
    import baddiffusion as cli

    def config(out, **opts):
        os.makedirs(out, exist_ok=True)
        return types.SimpleNamespace(output_dir=str(out), sample_ep=None, clip=True, seed=0, **opts)
    c = config(tmp_path / "plain")
    assert cli.quality_extra(c, None) == {}
    sc = cli.update_score_file(c, "score.json", None, 0.1, 0.2, extra={"inference_chunk": 8, **cli.quality_extra(c, None)})
    assert set(sc) == {"FID", "FID_reason", "MSE", "SSIM", "inference_chunk"}
    c = config(tmp_path / "flags", measure_prdc_k=5, measure_kid=True, kid_subset_size=50)
    sc = cli.update_score_file(c, "score.json", None, 0.1, 0.2, extra={"inference_chunk": 8, **cli.quality_extra(c, None)})
    assert set(sc) == {"FID", "FID_reason", "MSE", "SSIM", "inference_chunk", "precision", "recall", "density", "coverage", "PRDC_k", "KID_mean",
                       "KID_std", "KID_subsets", "KID_subset_size", "quality_reason"}
    assert all(sc[k] is None for k in ("precision", "recall", "density", "coverage", "KID_mean", "KID_std"))
    assert sc["PRDC_k"] == 5 and sc["KID_subsets"] == 100 and sc["KID_subset_size"] == 50 and "weights are absent" in sc["quality_reason"]
    assert sc == json.load(open(tmp_path / "flags" / "score.json"))
    c = config(tmp_path / "prdc", measure_prdc_k=3)
    assert set(cli.quality_extra(c, None)) == {"precision", "recall", "density", "coverage", "PRDC_k", "quality_reason"}
