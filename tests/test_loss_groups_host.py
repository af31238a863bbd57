"""CPU: bd_loss_groups_fwd_bwd checks its arguments on the host before any launch, so every rejected case fails loudly (negative
status + bd_last_error) in a process without a GPU; the workspace query; remove_backdoor's clean_target check."""
import ctypes
import math
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from baddiffusion_amd.build import build_lib
    build_lib(force=False, verbose=False)
    from baddiffusion_amd import _lib as L
    return L, L.load()


def desc(L, groups):
    d = L.LossGroupsDesc(n_groups=len(groups))
    for g, (r, w) in enumerate(groups[: L.LOSS_MAX_GROUPS]):
        d.group_rows[g], d.group_weight[g] = r, w
    return d


def call(L, lib, groups, rows=10, C=3, pred=0x1000, target=0x2000, losses=0x3000, ws=0x4000, ws_bytes=None, n_groups=None, gdesc="own"):
    """the pointers are never dereferenced: every case here must be turned away before a launch"""
    d = desc(L, groups)
    if n_groups is not None:
        d.n_groups = n_groups
    if ws_bytes is None:
        ws_bytes = lib.bd_loss_groups_workspace_bytes(L.LOSS_MAX_GROUPS)
    return lib.bd_loss_groups_fwd_bwd(pred, C, target, C, rows, C, 0, 1.0, ctypes.byref(d) if gdesc == "own" else None, losses, None, C, ws,
                                      ws_bytes, None)


def test_workspace_bytes_positive_for_every_group_count(lib):
    L, lib = lib
    assert L.LOSS_MAX_GROUPS == 4
    sizes = [lib.bd_loss_groups_workspace_bytes(n) for n in range(1, 5)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    assert lib.bd_loss_groups_workspace_bytes(0) == 0 and lib.bd_loss_groups_workspace_bytes(5) == 0


def test_struct_layout_matches_header(lib, tmp_path):
    L, _ = lib
    c = tmp_path / "s.c"
    c.write_text('#include <stdio.h>\n#include "bd_hip.h"\nint main(){printf("%zu %d\\n", sizeof(bd_loss_groups_desc), BD_LOSS_MAX_GROUPS);return 0;}')
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe])
    size, max_groups = subprocess.run([exe], capture_output=True, text=True).stdout.split()
    assert ctypes.sizeof(L.LossGroupsDesc) == int(size) and L.LOSS_MAX_GROUPS == int(max_groups)


@pytest.mark.parametrize("name,kwargs", [
    ("null pred", dict(groups=[(10, 1.0)], pred=None)),
    ("null target", dict(groups=[(10, 1.0)], target=None)),
    ("null losses", dict(groups=[(10, 1.0)], losses=None)),
    ("null workspace", dict(groups=[(10, 1.0)], ws=None)),
    ("null descriptor", dict(groups=[(10, 1.0)], gdesc=None)),
    ("no groups", dict(groups=[(10, 1.0)], n_groups=0)),
    ("negative group count", dict(groups=[(10, 1.0)], n_groups=-1)),
    ("five groups", dict(groups=[(2, 1.0)] * 4, n_groups=5)),
    ("zero rows in a group", dict(groups=[(10, 1.0), (0, 1.0)])),
    ("zero rows in the first group", dict(groups=[(0, 1.0), (10, 1.0)])),
    ("negative rows", dict(groups=[(11, 1.0), (-1, 1.0)])),
    ("rows sum short", dict(groups=[(4, 1.0), (5, 1.0)])),
    ("rows sum long", dict(groups=[(4, 1.0), (7, 1.0)])),
    ("negative weight", dict(groups=[(4, 1.0), (6, -0.5)])),
    ("nan weight", dict(groups=[(4, float("nan")), (6, 1.0)])),
    ("infinite weight", dict(groups=[(4, 1.0), (6, math.inf)])),
    ("workspace of one group for two", dict(groups=[(4, 1.0), (6, 1.0)], ws_bytes="one")),
    ("empty workspace", dict(groups=[(10, 1.0)], ws_bytes=0)),
])
def test_bad_arguments_are_rejected_without_gpu(lib, name, kwargs):
    L, lib = lib
    if kwargs.get("ws_bytes") == "one":
        kwargs = dict(kwargs, ws_bytes=lib.bd_loss_groups_workspace_bytes(1))
    status = call(L, lib, **kwargs)
    msg = lib.bd_last_error()
    assert status < 0, name
    assert msg and b"bd_loss_groups_fwd_bwd" in msg, (name, msg)


def test_bad_loss_type_is_rejected_without_gpu(lib):
    L, lib = lib
    d = desc(L, [(10, 1.0)])
    assert lib.bd_loss_groups_fwd_bwd(0x1000, 3, 0x2000, 3, 10, 3, 3, 1.0, ctypes.byref(d), 0x3000, None, 3, 0x4000, 1 << 20, None) < 0
    assert b"loss_type" in lib.bd_last_error()


def test_remove_backdoor_rejects_unknown_clean_target_before_touching_a_device():
    from baddiffusion_amd import defense
    clean = torch.zeros(8, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="clean_target"):
        defense.remove_backdoor(None, None, None, steps=1, batch=1, lr=1e-5, clean=clean, clean_batch=2, clean_target="bogus")
