"""CPU: the four K-split launchers (bd_conv3x3_ps, bd_conv3x3_ps_wgrad, bd_igemm, bd_gemm_sp) size their workspace exactly as their
bd_*_workspace_bytes functions report it, and the GroupNorm launchers (bd_gn_fwd, bd_gn_bwd) as bd_gn_plan reports it.  Each case hands
the launcher one byte less than the reported size: the call must be turned away with BD_ERR_WORKSPACE, and the need it prints must be
the reported size.  The check comes before any launch, so no GPU is involved; no call here is ever made with a sufficient workspace (the
pointers are fake).  bd_gn_workspace_bytes(B, C) is a bound over (HW, G), and is tested as one."""
import ctypes
import re

import pytest

BD_ERR_WORKSPACE = -4     # include/bd_hip.h
BD_OPK_DENSE = 0
P = [0x100000 * (i + 1) for i in range(6)]   # fake, 128-byte aligned, never dereferenced


@pytest.fixture(scope="module")
def lib():
    from baddiffusion_amd.build import build_lib
    build_lib(force=False, verbose=False)
    from baddiffusion_amd import _lib as L
    return L, L.load()


def conv_ps(L, B, H, W, K, N):
    return L.ConvPsDesc(B=B, H=H, W=W, K=K, N=N, direction=1, x_split=P[0], ldx=K, w_split=P[1], y=P[2], ldy=N, workspace=P[3])


def conv_ps_wgrad(L, B, H, W, Cin, Cout, db):
    return L.ConvPsWgradDesc(B=B, H=H, W=W, Cin=Cin, Cout=Cout, x_split=P[0], ldx=Cin, dy_split=P[1], lddy=Cout, dw=P[2],
                             db=P[4] if db else None, workspace=P[3])


def igemm(L, M, N, K, colsum):
    """C[M, N] = A^T B with both operands row-contiguous DENSE (what a_colsum needs): A is [K][M], B is [K][N]"""
    d = L.IgemmDesc(M=M, N=N, K=K, batch_outer=1, batch_inner=1, C=P[2], ldc=N, alpha=1.0, out_scale=1.0, workspace=P[3],
                    a_colsum=P[4] if colsum else None)
    d.A.kind, d.A.kc, d.A.p, d.A.ld = BD_OPK_DENSE, 0, P[0], M
    d.B.kind, d.B.kc, d.B.p, d.B.ld = BD_OPK_DENSE, 0, P[1], N
    return d


def gemm_sp(L, M, N, K, colsum):
    """a_colsum needs both operands K-major; without it the row-major form"""
    km = 1 if colsum else 0
    return L.GemmSpDesc(M=M, N=N, K=K, batch=1, a=P[0], lda=M if km else K, a_kmajor=km, b=P[1], ldb=N if km else K, b_kmajor=km,
                        c=P[2], ldc=N, alpha=1.0, out_scale=1.0, a_colsum=P[4] if colsum else None, workspace=P[3])


# (id, descriptor, size function, launcher, the "need" in the launcher's message).  The smallest shapes whose size is non-zero with one
# workgroup slot per CU on 256 CUs (also what a process without a device assumes), one per form that sizes differently.
CASES = [
    # 4 x 4 image, one 128 x 128 tile, 36 chunks of K: 9 splits of 4
    ("conv3x3_ps small split-K", lambda L: conv_ps(L, 1, 4, 4, 128, 128), "bd_conv3x3_ps_workspace_bytes", "bd_conv3x3_ps",
     r"split-K needs (\d+) workspace bytes"),
    # nine-tap form (W < 16), 16 chunks of 32 pixels: 2 splits of 8
    ("conv3x3_ps_wgrad nine taps", lambda L: conv_ps_wgrad(L, 32, 4, 4, 128, 128, True), "bd_conv3x3_ps_wgrad_workspace_bytes",
     "bd_conv3x3_ps_wgrad", r"workspace \d+ < (\d+)"),
    # shared-tap form (W >= 16): a third of the tiles on its own slot count
    ("conv3x3_ps_wgrad shared taps", lambda L: conv_ps_wgrad(L, 2, 16, 16, 128, 128, False), "bd_conv3x3_ps_wgrad_workspace_bytes",
     "bd_conv3x3_ps_wgrad", r"workspace \d+ < (\d+)"),
    # one 64 x 64 tile, 16 chunks of K: 2 splits of 8; with a_colsum 2 x M more floats behind the slabs
    ("igemm", lambda L: igemm(L, 4, 4, 512, False), "bd_igemm_workspace_bytes", "bd_igemm", r"split-K needs (\d+) workspace bytes"),
    ("igemm a_colsum", lambda L: igemm(L, 4, 4, 512, True), "bd_igemm_workspace_bytes", "bd_igemm", r"split-K needs (\d+) workspace bytes"),
    # one 128 x 128 tile, 32 chunks of K: 4 splits of 8
    ("gemm_sp", lambda L: gemm_sp(L, 128, 128, 1024, False), "bd_gemm_sp_workspace_bytes", "bd_gemm_sp", r"workspace \d+ < (\d+)"),
    ("gemm_sp a_colsum", lambda L: gemm_sp(L, 128, 128, 1024, True), "bd_gemm_sp_workspace_bytes", "bd_gemm_sp", r"workspace \d+ < (\d+)"),
]


@pytest.mark.parametrize("name,make,size_fn,launcher,need_re", CASES, ids=[c[0] for c in CASES])
def test_launcher_needs_what_its_size_function_reports(lib, name, make, size_fn, launcher, need_re):
    L, lib = lib
    d = make(L)
    size = getattr(lib, size_fn)(ctypes.byref(d))
    assert size > 0, name                       # (also keeps size - 1 from wrapping into a sufficient workspace)
    d.workspace_bytes = size - 1
    status = getattr(lib, launcher)(ctypes.byref(d), None)
    msg = lib.bd_last_error()
    assert status == BD_ERR_WORKSPACE, (name, status, msg)
    m = re.search(need_re.encode(), msg or b"")
    assert m, (name, msg)
    print(name, "size function", size, "launcher needs", int(m.group(1)))
    assert int(m.group(1)) == size, (name, msg)


def test_a_colsum_rows_lie_behind_the_igemm_slabs(lib):
    """the second region counts: 2 splits x M floats more than the slabs alone"""
    L, lib = lib
    plain = lib.bd_igemm_workspace_bytes(ctypes.byref(igemm(L, 4, 4, 512, False)))
    with_rows = lib.bd_igemm_workspace_bytes(ctypes.byref(igemm(L, 4, 4, 512, True)))
    assert plain == 2 * 4 * 4 * 4 and with_rows == plain + 2 * 4 * 4


# ---- GroupNorm: the launchers read the layout that bd_gn_plan reports (groupnorm.hip gn_fwd_workspace / gn_bwd_workspace) ----------------
def gn_plan(L, lib, B, HW, Cc, G, backward):
    p = L.GnPlanInfo()
    assert lib.bd_gn_plan(B, HW, Cc, G, backward, ctypes.byref(p)) == 0, lib.bd_last_error()
    return p


def gn_desc(L, B, HW, Cc, G, backward, params=True, partials=False):
    if not backward:
        return L.GnFwdDesc(B=B, HW=HW, C=Cc, G=G, eps=1e-5, silu=1, x=P[0], ldx=Cc, gamma=P[1], beta=P[2], y=P[3], ldy=Cc, mean=P[4], rstd=P[5],
                           workspace=P[0])
    return L.GnBwdDesc(B=B, HW=HW, C=Cc, G=G, silu=1, x=P[0], ldx=Cc, gamma=P[1], beta=P[2], mean=P[3], rstd=P[4], dy=P[5], lddy=Cc, dx=P[0],
                       lddx=Cc, dgamma=P[1] if params else None, dbeta=P[2] if params else None, workspace=P[3],
                       param_partials=P[4] if partials else None)


# (id, B, HW, C, G, backward, resident, the need worked out by hand from the layout in include/bd_hip.h)
GN_CASES = [
    ("gn_fwd two-stage", 2, 1024, 384, 32, 0, 0, 2 * 32 * 32 * 2 * 8),                           # S = 32: [B][S][G][2] fp64
    ("gn_bwd two-stage", 2, 1024, 384, 32, 1, 0, 2 * 32 * 384 * 3 * 4 + 2 * 32 * 2 * 4),        # [B][S][3][C] fp32 (1152 x 256) + [B][G][2] fp32
    ("gn_bwd two-stage S = 12", 40, 1024, 96, 8, 1, 0, 40 * 12 * 96 * 3 * 4 + 40 * 8 * 2 * 4),  # 552960 = 2160 x 256, then ds
    # S = 102 (512 // 5), 24 channels: the statistics rows are 5 * 102 * 24 * 3 * 4 = 146880 bytes = 573.75 x 256, so ds starts at 574 x 256
    ("gn_bwd two-stage, rounded rows", 5, 4096, 24, 6, 1, 0, 574 * 256 + 5 * 6 * 2 * 4),
    ("gn_bwd resident", 3, 64, 128, 32, 1, 1, 3 * 128 * 2 * 4),                                   # [B][2][C] fp32: the launcher folds the sums
]


@pytest.mark.parametrize("name,B,HW,Cc,G,backward,resident,by_hand", GN_CASES, ids=[c[0] for c in GN_CASES])
def test_gn_launcher_needs_what_its_plan_reports(lib, name, B, HW, Cc, G, backward, resident, by_hand):
    L, lib = lib
    p = gn_plan(L, lib, B, HW, Cc, G, backward)
    assert p.resident == resident and p.workspace_bytes == by_hand > 0, (name, p.resident, p.workspace_bytes, by_hand)
    d = gn_desc(L, B, HW, Cc, G, backward)
    d.workspace_bytes = p.workspace_bytes - 1
    status = (lib.bd_gn_bwd if backward else lib.bd_gn_fwd)(ctypes.byref(d), None)
    msg = lib.bd_last_error()
    assert status == BD_ERR_WORKSPACE, (name, status, msg)
    m = re.search(rb"workspace (\d+) < (\d+)", msg or b"")
    assert m, (name, msg)
    print(name, "plan", p.workspace_bytes, "launcher was given", int(m.group(1)), "and needs", int(m.group(2)))
    assert int(m.group(1)) == p.workspace_bytes - 1 and int(m.group(2)) == p.workspace_bytes, (name, msg)


def test_gn_resident_needs_a_workspace_only_for_the_sums_it_owns(lib):
    """the reported backward need is that of the largest descriptor variant: dgamma / dbeta wanted, no param_partials.  (With param_partials
    the same call passes the workspace check at 0 bytes and would launch: not made here.)"""
    L, lib = lib
    B, HW, Cc, G = 3, 64, 128, 32
    assert gn_plan(L, lib, B, HW, Cc, G, 1).workspace_bytes == B * Cc * 8
    assert gn_plan(L, lib, B, HW, Cc, G, 0).resident == 1 and gn_plan(L, lib, B, HW, Cc, G, 0).workspace_bytes == 0


# the shape grid of scripts/plan_step_helpers.py gnplans: every dispatch branch, and shapes the launchers turn away (skipped here)
GN_B = (1, 2, 3, 4, 5, 40, 128, 170, 171, 256, 257, 513, 515, 2048, 65535, 65536)
GN_HW = (16, 64, 256, 900, 1024, 2000, 4096, 4100, 65536)
GN_CG = ((24, 6), (64, 32), (96, 8), (128, 32), (256, 2), (256, 32), (384, 32), (512, 32), (768, 32), (1024, 32), (4096, 32), (4100, 4), (130, 32),
         (126, 6))


def test_gn_workspace_bytes_bounds_every_shape(lib):
    """bd_gn_workspace_bytes(B, C) >= the need of every (HW, G) the launchers take at that (B, C), in both directions"""
    L, lib = lib
    taken = tight = 0
    for B in GN_B:
        for HW in GN_HW:
            for Cc, G in GN_CG:
                p = L.GnPlanInfo()
                if lib.bd_gn_plan(B, HW, Cc, G, 0, ctypes.byref(p)) != 0:
                    continue
                bound = lib.bd_gn_workspace_bytes(B, Cc)
                need = max(p.workspace_bytes, gn_plan(L, lib, B, HW, Cc, G, 1).workspace_bytes)
                assert bound >= need, (B, HW, Cc, G, bound, need)
                taken += 1
                tight = max(tight, need / bound)
    print("shapes taken", taken, "of", len(GN_B) * len(GN_HW) * len(GN_CG), "largest need / bound", tight)
    assert taken > 1000
