"""CPU: the four K-split launchers (bd_conv3x3_ps, bd_conv3x3_ps_wgrad, bd_igemm, bd_gemm_sp) size their workspace exactly as their
bd_*_workspace_bytes functions report it.  Each case hands the launcher one byte less than the reported size: the call must be turned
away with BD_ERR_WORKSPACE, and the need it prints must be the reported size.  The check comes before any launch, so no GPU is involved;
no call here is ever made with a sufficient workspace (the pointers are fake)."""
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
