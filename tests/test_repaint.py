"""GPU: RePaint inpainting on the native path -- bd_repaint_step / bd_repaint_undo against the reference's vectors (tests/golden/repaint.npz,
written by make_golden_repaint.py from the imported diffusers RePaintScheduler / RePaintPipeline) and against an fp32 numpy restatement of
the two formulas in the kernels' stated order, their bit-exact properties, the shapes at which the launchers change path, the
trigger-consistent `shift` variant, RePaintScheduler / RePaintPipeline chains, and inpaint_eval.py.  Run with -m gpu on an MI355X."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_ref as U
from tests.golden import cases as C
from tests.golden import cases_repaint as CR

f32 = np.float32
TOL = 2e-6          # rtol = atol of test_ddpm_ddim_steps_golden, the sibling step kernels' bound


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def tables(gpu):
    """(betas, alphas_cumprod) as numpy fp32 and on the device"""
    from baddiffusion_amd.schedulers import RePaintScheduler
    s = RePaintScheduler()
    return s.betas.numpy(), s.alphas_cumprod.numpy(), s.betas.cuda(), s.alphas_cumprod.cuda()


def R(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def close(a, b, tol=TOL):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    np.testing.assert_allclose(a, b, rtol=tol, atol=tol)


def nhwc(x):
    """the same logical [N,C,H,W] tensor in NHWC storage"""
    return x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def step_np(ac, x, e, z, orig, mask, t, prev_t, eta, clip, shift=None):
    """bd_repaint_step's formula in its stated fp32 order on numpy arrays: (prev_sample, pred_original_sample)"""
    x, e, z = x.numpy(), e.numpy(), z.numpy()
    orig, mask = np.broadcast_to(orig.numpy(), x.shape), np.broadcast_to(mask.numpy(), x.shape)
    a_t = ac[t]
    a_p = ac[prev_t] if prev_t >= 0 else f32(1)
    x0 = (x - np.sqrt(f32(1) - a_t) * e) / np.sqrt(a_t)
    if clip:
        x0 = np.clip(x0, f32(-1), f32(1))
    sd = f32(eta) * np.sqrt(((f32(1) - a_p) / (f32(1) - a_t)) * (f32(1) - a_t / a_p))
    unknown = np.sqrt(a_p) * x0 + np.sqrt(f32(1) - a_p - sd * sd) * e
    if t > 0 and eta > 0:
        unknown = unknown + sd * z
    known = np.sqrt(a_p) * orig + np.sqrt(f32(1) - a_p) * z
    if shift is not None:
        known = known + (f32(1) - np.sqrt(a_p)) * np.broadcast_to(shift.numpy(), x.shape)
    out = mask * known + (f32(1) - mask) * unknown
    assert out.dtype == np.float32 and x0.dtype == np.float32
    return out, x0


def undo_np(betas, x, noises, t, shift=None):
    x = x.numpy()
    for i, z in enumerate(noises):
        b = betas[t + i]
        ca = np.sqrt(f32(1) - b)
        x = ca * x + np.sqrt(b) * z.numpy()
        if shift is not None:
            x = x + (f32(1) - ca) * np.broadcast_to(shift.numpy(), x.shape)
    assert x.dtype == np.float32
    return x


# ---------------------------------------------------------------------------------------------------- against the fixtures
def test_step_matches_the_reference(gpu, golden, tables):
    from baddiffusion_amd.schedulers import RePaintScheduler
    g = golden("repaint")
    _, ac, _, _ = tables
    x, e, orig = CR.step_inputs()
    z = torch.from_numpy(g["step_noise"])
    assert torch.equal(z, torch.randn(x.shape, generator=torch.Generator().manual_seed(CR.STEP_NOISE_SEED)))
    for clip in (True, False):
        s = RePaintScheduler(clip_sample=clip)
        s.set_timesteps(CR.STEP_INFER)
        for t in CR.STEP_TS:
            for eta in CR.STEP_ETAS:
                s.eta = eta
                for kind in CR.STEP_MASKS:
                    mask = CR.step_mask(kind)
                    want = g[f"step_{t}_{int(clip)}_{eta}_{kind}_prev"]
                    # noise drawn by the scheduler from the generator, as the reference draws it
                    r = s.step(e.cuda(), t, x.cuda(), orig.cuda(), mask.cuda(), generator=torch.Generator().manual_seed(CR.STEP_NOISE_SEED))
                    close(r.prev_sample, want)
                    close(r.pred_original_sample, g[f"step_{t}_{int(clip)}_x0"])
                    # the numpy restatement the other tests lean on agrees with the reference too
                    p_np, x0_np = step_np(ac, x, e, z, orig, mask, t, t - 100, eta, clip)
                    close(p_np, want)
                    close(x0_np, g[f"step_{t}_{int(clip)}_x0"])
    prev, x0 = s.step(e.cuda(), 500, x.cuda(), orig.cuda(), mask.cuda(), noise=z.cuda(), return_dict=False)
    close(prev, g[f"step_500_0_1.0_frac_prev"])


def test_undo_matches_the_reference(gpu, golden, tables):
    from baddiffusion_amd.schedulers import RePaintScheduler
    g = golden("repaint")
    betas, _, _, _ = tables
    x = CR.undo_sample()
    for tag, (n, t) in CR.UNDO_CASES.items():
        s = RePaintScheduler()
        s.set_timesteps(n)
        noises = list(torch.from_numpy(g[f"undo_{tag}_noise"]))
        assert len(noises) == 1000 // n
        close(s.undo_step(x.cuda(), t, generator=torch.Generator().manual_seed(CR.UNDO_NOISE_SEED)), g[f"undo_{tag}"])
        close(s.undo_step(x.cuda(), t, noise=[z.cuda() for z in noises]), g[f"undo_{tag}"])
        close(undo_np(betas, x, noises, t), g[f"undo_{tag}"])
        with pytest.raises(ValueError):
            s.undo_step(x.cuda(), t, noise=[z.cuda() for z in noises[:-1]])


# ---------------------------------------------------------------------------------------------------- bit-exact properties
def test_step_bit_exact_properties(gpu, tables):
    from baddiffusion_amd import ops
    _, _, _, acd = tables
    x, e, orig = (t.cuda() for t in CR.step_inputs())
    z = R(5, 2, 3, 8, 8).cuda()
    frac = CR.step_mask("frac").cuda()
    shift = CR.shift_image().cuda()
    kw = dict(eta=0.5, clip_sample=True)
    # mask == 0: the DDIM step, bit for bit
    for t, prev_t, eta in ((500, 400, 0.5), (900, 800, 0.0), (900, 800, 1.0), (0, -100, 1.0)):
        got = ops.repaint_step(e, x, z, orig, torch.zeros(1, 1, 8, 8).cuda(), acd, t, prev_t, eta=eta)
        want = ops.ddim_step(e, x, acd, t, prev_t, eta=eta, noise=z, final_alpha_cumprod=1.0)
        assert torch.equal(got, want), (t, eta)
    # mask == 1 where alpha_prod_prev = 1: the original image, bit for bit
    for eta in (0.0, 1.0):
        got = ops.repaint_step(e, x, z, orig, torch.ones(1, 1, 8, 8).cuda(), acd, 0, -100, eta=eta)
        assert torch.equal(got, orig)
    # NCHW storage and NHWC storage give the same bits
    base, base_x0 = ops.repaint_step(e, x, z, orig, frac, acd, 500, 400, shift=shift, want_x0=True, **kw)
    assert base.is_contiguous()
    got, got_x0 = ops.repaint_step(nhwc(e), nhwc(x), nhwc(z), orig, frac, acd, 500, 400, shift=shift, want_x0=True, **kw)
    assert got.permute(0, 2, 3, 1).is_contiguous() and torch.equal(got, base) and torch.equal(got_x0, base_x0)
    got = ops.repaint_step(nhwc(e), nhwc(x), nhwc(z), nhwc(orig), nhwc(frac), acd, 500, 400, shift=shift, **kw)
    assert torch.equal(got, base)
    got = ops.repaint_step(e, nhwc(x), z, orig, frac, acd, 500, 400, shift=shift, **kw)     # mixed layouts are brought to sample's
    assert torch.equal(got, base)
    # pred_original requested or not: the same prev
    assert torch.equal(ops.repaint_step(e, x, z, orig, frac, acd, 500, 400, shift=shift, want_x0=False, **kw), base)
    # stride-0 operands give the bits of the materialised ones
    for o, m, s in ((orig[:1], CR.step_mask("one").cuda(), shift), (orig[0], CR.step_mask("row").cuda(), shift[None]),
                    (orig[:, :1], frac[:1], shift[:, :, :1]), (orig, frac[0], shift[:1, :1, :1])):
        for lay in (lambda t: t, nhwc):
            a = ops.repaint_step(lay(e), lay(x), lay(z), o, m, acd, 500, 400, shift=s, **kw)
            full = [t.expand(2, 3, 8, 8).contiguous() for t in (o, m, s)]
            b = ops.repaint_step(lay(e), lay(x), lay(z), full[0], full[1], acd, 500, 400, shift=full[2], **kw)
            assert torch.equal(a, b)
            got = ops.repaint_undo(lay(x), [lay(z), lay(e)], tables[2], 400, shift=s)
            assert torch.equal(got, ops.repaint_undo(lay(x), [lay(z), lay(e)], tables[2], 400, shift=full[2]))


# ---------------------------------------------------------------------------------------------------- shapes that change the path
BIG = (3, 3, 512, 512)          # 589 824 float4 = 2 304 blocks of 256 > the 2 048-block grid: the grid-stride loop runs twice
SHAPES = {"scalar_tail_1x3x5x7": (1, 3, 5, 7), "unaligned_view": (2, 3, 8, 8), "vector_2x3x8x8": (2, 3, 8, 8), "two_grid_passes": BIG}


@pytest.mark.parametrize("name", list(SHAPES))
def test_step_and_undo_shapes(gpu, tables, name):
    """every launcher path against the fp32 restatement: one element per thread with a ragged last block (105 elements), a view 4 bytes
    into a larger buffer (not 16-byte aligned: scalar path), the 16-byte path, and more float4s than one pass of the capped grid covers;
    broadcast original / mask / shift throughout, both storage orders"""
    from baddiffusion_amd import ops
    betas, ac, bd_, acd = tables
    shape = SHAPES[name]
    N, Cc, H, W = shape
    x, e, z, z2 = (R(200 + i, *shape) for i in range(4))
    orig = torch.rand(1, Cc, H, W, generator=torch.Generator().manual_seed(210)) * 2 - 1
    mask = (torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(211)) < 0.5).float()
    mask[..., 0] = 0.25                                                                         # not binary
    shift = torch.rand(Cc, H, W, generator=torch.Generator().manual_seed(212))

    def put(t):
        if name != "unaligned_view":
            return t.cuda()
        buf = torch.empty(t.numel() + 1, device="cuda")
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v

    layouts = (lambda t: t,) if name in ("unaligned_view", "two_grid_passes") else (lambda t: t, nhwc)
    for lay in layouts:
        for sh in (None, shift):
            want, want_x0 = step_np(ac, x, e, z, orig, mask, 500, 400, 0.5, True, shift=sh)
            got, got_x0 = ops.repaint_step(lay(put(e)), lay(put(x)), lay(put(z)), orig.cuda(), mask.cuda(), acd, 500, 400, eta=0.5, clip_sample=True,
                                           shift=None if sh is None else sh.cuda(), want_x0=True)
            close(got, want)
            close(got_x0, want_x0)
            got = ops.repaint_undo(lay(put(x)), [lay(put(z)), lay(put(z2))], bd_, 400, shift=None if sh is None else sh.cuda())
            close(got, undo_np(betas, x, [z, z2], 400, shift=sh))


# ---------------------------------------------------------------------------------------------------- undo
@pytest.mark.parametrize("k", [1, 4, 8, 9, 19])
def test_undo_chunks_equal_single_calls(gpu, tables, k):
    """k = 1, one launch (4, and the per-launch limit 8), and above the limit (9 = 8 + 1, 19 = 8 + 8 + 3): equal to the restatement, and
    bit for bit to k calls with one noise each, with and without shift, in both storage orders and on the scalar path"""
    from baddiffusion_amd import _lib as L
    from baddiffusion_amd import ops
    assert L.REPAINT_UNDO_MAX == 8
    betas, _, bd_, _ = tables
    shift = CR.shift_image()
    for shape in ((2, 3, 8, 8), (1, 3, 5, 7)):
        x = R(300, *shape)
        noises = [R(301 + i, *shape) for i in range(k)]
        sh = shift[:, :shape[2], :shape[3]]
        for s in (None, sh):
            sd = None if s is None else s.cuda()
            for lay in (lambda t: t, nhwc):
                got = ops.repaint_undo(lay(x.cuda()), [lay(z.cuda()) for z in noises], bd_, 700, shift=sd)
                close(got, undo_np(betas, x, noises, 700, shift=s))
                one = lay(x.cuda())
                for i, z in enumerate(noises):
                    one = ops.repaint_undo(one, [lay(z.cuda())], bd_, 700 + i, shift=sd)
                assert torch.equal(got, one)
    # in place
    buf = x.cuda()
    want = ops.repaint_undo(buf, [z.cuda() for z in noises], bd_, 700)
    assert ops.repaint_undo(buf, [z.cuda() for z in noises], bd_, 700, out=buf) is buf and torch.equal(buf, want)
    with pytest.raises(RuntimeError, match="bd_repaint_undo"):
        ops.repaint_undo(buf, [z.cuda() for z in noises], bd_, 1000 - k + 1)


# ---------------------------------------------------------------------------------------------------- shift
def test_shift_variant(gpu, tables):
    from baddiffusion_amd import ops
    from baddiffusion_amd.schedulers import RePaintScheduler
    betas, ac, bd_, acd = tables
    x, e, orig = CR.step_inputs()
    z, z2 = R(5, 2, 3, 8, 8), R(6, 2, 3, 8, 8)
    mask, shift = CR.step_mask("frac"), CR.shift_image()
    s = RePaintScheduler()
    s.set_timesteps(10)
    for t in CR.STEP_TS:
        for eta in (0.0, 1.0):
            s.eta = eta
            got = s.step(e.cuda(), t, x.cuda(), orig.cuda(), mask.cuda(), noise=z.cuda(), shift=shift.cuda()).prev_sample
            close(got, step_np(ac, x, e, z, orig, mask, t, t - 100, eta, True, shift=shift)[0])
            none = s.step(e.cuda(), t, x.cuda(), orig.cuda(), mask.cuda(), noise=z.cuda()).prev_sample
            zero = s.step(e.cuda(), t, x.cuda(), orig.cuda(), mask.cuda(), noise=z.cuda(), shift=torch.zeros_like(shift).cuda()).prev_sample
            assert torch.equal(none, zero)                                      # a zero shift equals none (x + 0 * c)
            if t > 0:
                assert not torch.equal(got, none)
    # at the final step (alpha_prod_prev = 1, so 1 - sqrt(alpha_prod_prev) = 0) the known region is the original with or without it
    binary = CR.step_mask("one")
    known = binary.expand(2, 3, 8, 8) == 1
    for sh in (None, shift.cuda()):
        got = s.step(e.cuda(), 0, x.cuda(), orig.cuda(), binary.cuda(), noise=z.cuda(), shift=sh).prev_sample.cpu()
        assert torch.equal(got[known], orig[known])
    s.set_timesteps(500)                                                        # two sub-steps per undo
    got = s.undo_step(x.cuda(), 400, noise=[z.cuda(), z2.cuda()], shift=shift.cuda())
    close(got, undo_np(betas, x, [z, z2], 400, shift=shift))
    assert torch.equal(s.undo_step(x.cuda(), 400, noise=[z.cuda(), z2.cuda()]),
                       s.undo_step(x.cuda(), 400, noise=[z.cuda(), z2.cuda()], shift=torch.zeros(3, 8, 8).cuda()))
    # the point of the variant: x - (1 - sqrt(a)) R of a poisoned sample follows the plain process.  A sample shifted by (1 - sqrt(a)) R,
    # undone with shift = R, is the plain undo shifted by (1 - sqrt(a'))  R, a' = a (1 - beta_400) (1 - beta_401): exact algebra, so the
    # two sides differ by fp32 rounding alone: 11 roundings (the shifted input, 2 x 3 operations, 2 x 2 in the plain run) of values
    # below 8, at most 2^-21 each = 5.2e-6
    a = np.float64(ac[400])
    a2 = a * (1 - np.float64(betas[400])) * (1 - np.float64(betas[401]))
    shifted = (x.double() + (1 - np.sqrt(a)) * shift.double()).float().cuda()
    plain = s.undo_step(x.cuda(), 400, noise=[z.cuda(), z2.cuda()]).cpu()
    np.testing.assert_allclose(s.undo_step(shifted, 400, noise=[z.cuda(), z2.cuda()], shift=shift.cuda()).cpu().double().numpy(),
                               (plain.double() + (1 - np.sqrt(a2)) * shift.double()).numpy(), rtol=0, atol=5.2e-6)


# ---------------------------------------------------------------------------------------------------- chains
@pytest.mark.parametrize("eta,clip", CR.CHAIN_CASES)
def test_stand_in_chain(gpu, golden, eta, clip):
    """The pipeline loop of (10, 2, 3) with cases.pndm_fake_model in place of the UNet: 26 steps and 16 undo transitions of 100 sub-steps.
    Every intermediate sample within max(4e-6, 4 * chain_dev64) * max|ref| of the reference's, where chain_dev64 is the reference's own
    distance from the same recurrence in fp64 (recorded in the fixture: 1.6e-6 .. 2.6e-6)."""
    from baddiffusion_amd.schedulers import RePaintScheduler
    g = golden("repaint")
    tag = f"{eta}_{int(clip)}"
    ref, dev64 = g[f"chain_{tag}"], float(g[f"chain_dev64_{tag}"])
    bound = max(4e-6, 4 * dev64)
    x, orig, mask = (t.cuda() for t in CR.chain_inputs())
    s = RePaintScheduler(clip_sample=clip)
    s.set_timesteps(*CR.CHAIN)
    s.eta = eta
    gen = torch.Generator().manual_seed(CR.CHAIN_SEED)
    ts = [int(t) for t in s.timesteps]
    assert len(ts) == len(ref) == 42
    t_last, worst = ts[0] + 1, 0.0
    for i, t in enumerate(ts):
        if t < t_last:
            x = s.step(C.pndm_fake_model(x, t), t, x, orig, mask, generator=gen).prev_sample
        else:
            x = s.undo_step(x, t_last, generator=gen)
        t_last = t
        dev = float(np.abs(x.cpu().numpy() - ref[i]).max() / np.abs(ref[i]).max())
        worst = max(worst, dev)
        assert dev <= bound, (i, t, dev, bound)
    print(f"MEASURE repaint stand-in chain eta={eta} clip={clip}: worst step deviation {worst:.3e}, bound {bound:.3e} (reference vs fp64 {dev64:.3e})")


def make_model(cfg, seed):
    from baddiffusion_amd.unet import unet_from_config
    m = unet_from_config(cfg).cuda()
    m.load_state_dict(U.gen_params(cfg, seed))
    return m


@pytest.fixture(scope="module")
def small_pipe(gpu):
    from baddiffusion_amd.pipelines import RePaintPipeline
    from baddiffusion_amd.schedulers import DDPMScheduler, RePaintScheduler
    pipe = RePaintPipeline(unet=make_model(C.SMALL_CFGS[CR.UNET_CFG], CR.UNET_PARAM_SEED), scheduler=DDPMScheduler(clip_sample=True))
    assert type(pipe.scheduler) is RePaintScheduler
    return pipe


@pytest.mark.parametrize("eta", CR.UNET_ETAS)
def test_unet_chain_vs_reference_images(gpu, golden, small_pipe, eta):
    """the reference RePaintPipeline on the small UNet: (4, 1, 2), 7 evaluations and 3 undo transitions of 250 sub-steps"""
    ref = golden("repaint")[f"unet_{eta}_images"]                                   # [2,16,16,3] in [0, 1]
    image, mask = CR.unet_inputs()
    hole = ref[(slice(None),) + CR.UNET_HOLE]
    assert ((hole == 0) | (hole == 1)).mean() < 0.5                                 # the comparison is not one of saturated pixels
    n, jl, js = CR.UNET_CHAIN
    r = small_pipe(image, mask, num_inference_steps=n, eta=eta, jump_length=jl, jump_n_sample=js,
                   generator=torch.Generator().manual_seed(CR.UNET_SEED), output_type=None)
    assert r.images.shape == (2, 16, 16, 3) and r.images.dtype == np.float32
    known = np.broadcast_to(mask.permute(0, 2, 3, 1).numpy() == 1, r.images.shape)
    want_known = (image / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(r.images[known], want_known[known])                       # the known region is the original, exactly
    print(f"MEASURE repaint unet chain eta={eta}: max |image - ref| {np.abs(r.images - ref).max():.3e}")
    np.testing.assert_allclose(r.images, ref, rtol=1e-3, atol=2e-4)


# ---------------------------------------------------------------------------------------------------- pipeline surface
def test_pipeline_surface(gpu, small_pipe):
    image, mask = CR.unet_inputs()
    kw = dict(num_inference_steps=3, jump_length=1, jump_n_sample=2)
    ts = small_pipe._counts(3, 1, 2)
    init = R(400, 2, 3, 16, 16)
    r = small_pipe(image, mask, init=init, output_type=None, save_every_step=True, **kw)
    assert len(r.movie) == 1 + sum(ts) and r.movie[0].shape == (2, 16, 16, 3)
    np.testing.assert_array_equal(r.movie[0], (init / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).numpy())
    np.testing.assert_array_equal(r.movie[-1], r.images)
    # init= replaces the initial draw: eta = 0 at (3, 1, 2) still draws in step and undo, so fix the stream too
    a = small_pipe(image, mask, init=init, output_type=None, generator=torch.Generator().manual_seed(1), **kw).images
    b = small_pipe(image, mask, init=init, output_type=None, generator=torch.Generator().manual_seed(1), **kw).images
    c = small_pipe(image, mask, init=init + 0.5, output_type=None, generator=torch.Generator().manual_seed(1), **kw).images
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    g = torch.Generator().manual_seed(1)
    first = torch.randn(2, 3, 16, 16, generator=g)                                   # what the pipeline draws when init is not given
    d = small_pipe(image, mask, output_type=None, generator=torch.Generator().manual_seed(1), **kw).images
    e = small_pipe(image, mask, init=first, output_type=None, generator=g, **kw).images
    assert np.array_equal(d, e)
    # u8
    u8 = small_pipe(image, mask, init=init, output_type="u8", generator=torch.Generator().manual_seed(1), **kw).images
    assert u8.is_cuda and u8.dtype == torch.uint8 and tuple(u8.shape) == (2, 16, 16, 3)
    assert np.abs(u8.cpu().numpy().astype(np.float64) - a.astype(np.float64) * 255).max() <= 0.5 + 1e-4     # the float image, rounded
    pil = small_pipe(image, mask, init=init, **kw).images
    assert len(pil) == 2 and pil[0].size == (16, 16)
    # one [C,H,W] image shared by all chains: the same as the expanded batch
    shared = small_pipe(image[0], mask, init=init, output_type=None, generator=torch.Generator().manual_seed(1), **kw).images
    full = small_pipe(image[:1].expand(2, 3, 16, 16), mask, init=init, output_type=None, generator=torch.Generator().manual_seed(1), **kw).images
    assert np.array_equal(shared, full)
    four = small_pipe(image[0], mask[0, 0], batch_size=4, output_type=None, **kw).images
    assert four.shape == (4, 16, 16, 3)
    # known_shift changes the chain but not the known region of the result
    tau = torch.zeros(3, 16, 16); tau[:, 12:, 12:] = 1.5
    k = small_pipe(image, mask, init=init, known_shift=tau, output_type=None, generator=torch.Generator().manual_seed(1), **kw).images
    known = np.broadcast_to(mask.permute(0, 2, 3, 1).numpy() == 1, a.shape)
    assert np.array_equal(k[known], a[known]) and not np.array_equal(k, a)
    with pytest.raises(ValueError):
        small_pipe(image, mask, init=R(1, 3, 3, 16, 16), **kw)


def test_backdoor_scores_through_the_inpainting_pipeline(gpu, small_pipe):
    from baddiffusion_amd.defense import backdoor_scores
    image, mask = CR.unet_inputs()
    tau = (0.5 * R(12, 3, 16, 16)).cuda()
    sc = backdoor_scores(small_pipe, tau, n=4, image=image[0], mask_image=mask, num_inference_steps=3, jump_length=1, jump_n_sample=2)
    assert set(sc) == {"uniformity_clean", "uniformity_trigger", "tv_clean", "tv_trigger", "uniformity_ratio"}
    assert all(isinstance(v, float) and math.isfinite(v) for v in sc.values()), sc


def test_inpaint_eval_main(gpu, tmp_path):
    import inpaint_eval as E
    from baddiffusion_amd.model import save_scheduler, save_unet
    from baddiffusion_amd.schedulers import DDPMScheduler
    ckpt = str(tmp_path / "ckpt_small")
    save_unet(make_model(C.SMALL_CFGS["small"], 7), os.path.join(ckpt, "unet"))
    save_scheduler(DDPMScheduler(), os.path.join(ckpt, "scheduler"))
    common = ["--ckpt", ckpt, "--n", "4", "--batch", "2", "--infer_steps", "4", "--jump_length", "1", "--jump_n_sample", "2"]
    base_keys = {"hole_share", "mse_clean", "mse_trigger", "ssim_clean", "ssim_trigger"}
    result = E.main(common + ["--output_dir", str(tmp_path / "plain"), "--mask", "box"])
    out = os.path.join(str(tmp_path / "plain"), "res_inpaint_box_is4_j1x2_eta0.0_ckpt_small")
    score = json.load(open(os.path.join(out, "score.json")))
    assert score == json.loads(json.dumps(result)) and set(score) == base_keys
    assert all(isinstance(v, float) and math.isfinite(v) for v in score.values()), score
    assert score["hole_share"] == 0.25 and score["mse_clean"] > 0 and -1.0 <= score["ssim_clean"] <= 1.0
    from PIL import Image
    for tag in ("clean", "trigger"):
        assert Image.open(os.path.join(out, f"{tag}.png")).size == (32, 32)          # 4 images of 16 x 16
    result = E.main(common + ["--output_dir", str(tmp_path / "known"), "--mask", "half", "--eta", "1.0", "--target", "CORNER", "--asr_threshold", "0.5",
                              "--consistent"])
    out = os.path.join(str(tmp_path / "known"), "res_inpaint_half_is4_j1x2_eta1.0_consistent_ckpt_small")
    score = json.load(open(os.path.join(out, "score.json")))
    assert score == json.loads(json.dumps(result))
    assert set(score) == base_keys | {f"{k}_{tag}" for k in ("mse_target", "ssim_target", "asr") for tag in ("clean", "trigger")}
    assert all(isinstance(v, float) and math.isfinite(v) for v in score.values()), score
    assert score["hole_share"] == 0.5 and 0.0 <= score["asr_clean"] <= 1.0 and 0.0 <= score["asr_trigger"] <= 1.0
