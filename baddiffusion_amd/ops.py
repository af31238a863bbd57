"""Thin Python wrappers over the C ABI (include/bd_hip.h): torch tensors in, torch tensors out.

Tensors are only carriers of device memory here (allocation, streams); every FLOP on the hot path
happens in libbd_hip.so.  All wrappers enqueue on torch's current stream and never synchronise.
Activations are NHWC: a [B,H,W,C] contiguous tensor, or any 2-D [rows, C] view with row stride `ld`.
"""
import ctypes as C

import torch

from . import _lib as L

_ws_cache = {}


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("baddiffusion_amd.ops: tensors must live on the GPU (no CPU fallback on the hot path)")


def workspace(nbytes, device, tag="default"):
    """A cached scratch buffer of at least nbytes (per device / tag)."""
    key = (str(device), tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def _ld(t):
    """leading dimension (elements between rows) of a [..., C] tensor whose last dim is contiguous."""
    assert t.size(-1) == 1 or t.stride(-1) == 1     # (the stride of a size-1 dimension is arbitrary)
    return t.stride(-2) if t.dim() >= 2 else t.shape[-1]


# ------------------------------------------------------------------------------------------------ a-1/a-2
def poison_qsample(images, is_poison, trigger, target_img, noise, timesteps, alphas, alphas_cumprod,
                   vmin=-1.0, want_batch=False, want_mask=False, want_image=False, row_index=None, flip=None, corr=None):
    """Fused blend + q_sample.  images: float [B,C,H,W] (normalised) or uint8 [B,H,W,C].
    row_index (int64 [B]): batch row b reads images[row_index[b]] (images is then the whole resident array);
    flip (bool/uint8 [B]): mirror that image along W.  Both optional: the shuffled gather and
    RandomHorizontalFlip of the reference's DataLoader, fused into the kernel.
    corr (float32 [T], device): target = corr[t] R + eps (bd_poison_qsample_corr; correction.make_table) in place of the in-kernel
    rho_t; None is bd_poison_qsample.
    Returns (x_noisy NHWC [B,H,W,C], target NHWC [B,H,W,C][, R NCHW, x0 NCHW][, mask int64 [C,H,W]])."""
    lib = L.load()
    _need_cuda(images, is_poison, trigger, target_img, noise, timesteps, alphas, alphas_cumprod, row_index, flip)
    u8 = images.dtype == torch.uint8
    if u8:
        B, H, W, Cc = images.shape
    else:
        B, Cc, H, W = images.shape
    if row_index is not None:
        row_index = row_index.to(torch.int64).contiguous()
        B = row_index.numel()
    if flip is not None:
        flip = flip.to(torch.uint8).contiguous()
        assert flip.numel() == B
    dev = images.device
    images = images.contiguous(); noise = noise.contiguous()
    is_poison = is_poison.to(torch.uint8).contiguous()
    trigger = trigger.contiguous().float(); target_img = target_img.contiguous().float()
    timesteps = timesteps.to(torch.int64).contiguous()
    xn = torch.empty(B, H, W, Cc, device=dev); tg = torch.empty(B, H, W, Cc, device=dev)
    R = torch.empty(B, Cc, H, W, device=dev) if want_batch else None
    x0 = torch.empty(B, Cc, H, W, device=dev) if want_batch else None
    mask = torch.empty(Cc, H, W, dtype=torch.int64, device=dev) if want_mask else None
    image = torch.empty(B, Cc, H, W, device=dev) if want_image else None
    kw = dict(B=B, C=Cc, H=H, W=W, images_f32=None if u8 else L.ptr(images),
              images_u8=L.ptr(images) if u8 else None, is_poison=L.ptr(is_poison),
              trigger=L.ptr(trigger), target_img=L.ptr(target_img), noise=L.ptr(noise),
              timesteps=L.ptr(timesteps), alphas=L.ptr(alphas), alphas_cumprod=L.ptr(alphas_cumprod),
              vmin=vmin, x_noisy=L.ptr(xn), ld_noisy=Cc, target=L.ptr(tg), ld_target=Cc,
              R_out=L.ptr(R), x0_out=L.ptr(x0), mask_out=L.ptr(mask), image_out=L.ptr(image),
              row_index=L.ptr(row_index), flip=L.ptr(flip))
    if corr is None:
        d = L.PoisonQsampleDesc(**kw)
        L.check(lib.bd_poison_qsample(C.byref(d), L.stream()), "bd_poison_qsample")
    else:
        corr = _corr_table(corr, alphas_cumprod)
        d = L.PoisonQsampleCorrDesc(corr=L.ptr(corr), **kw)
        L.check(lib.bd_poison_qsample_corr(C.byref(d), L.stream()), "bd_poison_qsample_corr")
    out = [xn, tg]
    if want_batch:
        out += [R, x0]
    if want_mask:
        out += [mask]
    if want_image:
        out += [image]
    return tuple(out)


def _corr_table(corr, alphas_cumprod):
    """the target-coefficient table of the *_corr entry points: float32, contiguous, on the GPU, one entry per timestep"""
    _need_cuda(corr)
    if corr.dtype != torch.float32 or corr.dim() != 1 or corr.numel() != alphas_cumprod.numel():
        raise ValueError(f"corr must be a float32 [T = {alphas_cumprod.numel()}] table, got {corr.dtype} {tuple(corr.shape)}")
    return corr.contiguous()


def qsample(x0, R, noise, timesteps, alphas, alphas_cumprod, corr=None):
    """loss.py:257-285 on NCHW inputs -> (x_noisy, target) NHWC [B,H,W,C].  corr: as in poison_qsample (bd_qsample_corr)."""
    lib = L.load()
    _need_cuda(x0, R, noise, timesteps, alphas, alphas_cumprod)
    B, Cc, H, W = x0.shape
    x0 = x0.contiguous().float(); R = R.contiguous().float(); noise = noise.contiguous().float()
    timesteps = timesteps.to(torch.int64).contiguous()
    xn = torch.empty(B, H, W, Cc, device=x0.device); tg = torch.empty(B, H, W, Cc, device=x0.device)
    kw = dict(B=B, C=Cc, H=H, W=W, x0=L.ptr(x0), R=L.ptr(R), noise=L.ptr(noise), timesteps=L.ptr(timesteps),
              alphas=L.ptr(alphas), alphas_cumprod=L.ptr(alphas_cumprod), x_noisy=L.ptr(xn), ld_noisy=Cc,
              target=L.ptr(tg), ld_target=Cc)
    if corr is None:
        d = L.QsampleDesc(**kw)
        L.check(lib.bd_qsample(C.byref(d), L.stream()), "bd_qsample")
    else:
        corr = _corr_table(corr, alphas_cumprod)
        d = L.QsampleCorrDesc(corr=L.ptr(corr), **kw)
        L.check(lib.bd_qsample_corr(C.byref(d), L.stream()), "bd_qsample_corr")
    return xn, tg


def nchw_to_nhwc(x):
    lib = L.load(); _need_cuda(x)
    B, Cc, H, W = x.shape
    x = x.contiguous().float()
    y = torch.empty(B, H, W, Cc, device=x.device)
    L.check(lib.bd_nchw_to_nhwc(L.ptr(x), L.ptr(y), B, Cc, H, W, Cc, L.stream()), "bd_nchw_to_nhwc")
    return y


def nhwc_to_nchw(x):
    lib = L.load(); _need_cuda(x)
    B, H, W, Cc = x.shape
    x = x.contiguous()
    y = torch.empty(B, Cc, H, W, device=x.device)
    L.check(lib.bd_nhwc_to_nchw(L.ptr(x), Cc, L.ptr(y), B, Cc, H, W, L.stream()), "bd_nhwc_to_nchw")
    return y


# ------------------------------------------------------------------------------------------------ a-5/a-6/a-7
def _threshold_fields(who, sample, x0_quantile, sample_max_value):
    """the three dynamic-thresholding fields of a step descriptor; x0_quantile None switches the branch off"""
    if x0_quantile is None:
        return dict(x0_quantile=None, image_elems=0, sample_max_value=1.0)
    _need_cuda(x0_quantile)
    if x0_quantile.dtype != torch.float32 or x0_quantile.dim() != 1 or not x0_quantile.is_contiguous() \
            or x0_quantile.numel() != sample.shape[0]:
        raise ValueError(f"{who}: x0_quantile must be a contiguous float32 [{sample.shape[0]}] tensor, one value per image")
    return dict(x0_quantile=L.ptr(x0_quantile), image_elems=sample.numel() // sample.shape[0], sample_max_value=float(sample_max_value))


def ddpm_step(model_output, sample, noise, alphas_cumprod, t, prev_t, variance_type="fixed_small", clip_sample=True,
              clip_sample_range=1.0, clip_defense=False, clip_defense_range=1.0, out=None, want_x0=False, x0_quantile=None,
              sample_max_value=1.0):
    """x0_quantile ([B] raw quantiles of |x0|, from abs_quantile): dynamic thresholding of the predicted x0 in place of clip_sample;
    the tensors' dimension 0 must then be the outermost in memory (both layouts of the schedulers are)"""
    lib = L.load(); _need_cuda(model_output, sample, noise, alphas_cumprod)
    vt = {"fixed_small": 0, "fixed_large": 1}.get(variance_type)
    if vt is None:
        raise NotImplementedError(f"variance_type {variance_type} is not supported by the HIP DDPM step "
                                  "(BadDiffusion uses fixed_small / fixed_large)")
    assert model_output.is_contiguous() and sample.is_contiguous()
    prev = torch.empty_like(sample) if out is None else out
    x0 = torch.empty_like(sample) if want_x0 else None
    d = L.DdpmStepDesc(n=sample.numel(), model_output=L.ptr(model_output), sample=L.ptr(sample),
                       noise=L.ptr(noise.contiguous()) if noise is not None else None, prev_sample=L.ptr(prev),
                       pred_original=L.ptr(x0), alphas_cumprod=L.ptr(alphas_cumprod), t=int(t), prev_t=int(prev_t),
                       variance_type=vt, clip_sample=int(bool(clip_sample)), clip_sample_range=clip_sample_range,
                       clip_defense=int(bool(clip_defense)), clip_defense_range=clip_defense_range,
                       **_threshold_fields("ddpm_step", sample, x0_quantile, sample_max_value))
    L.check(lib.bd_ddpm_step(C.byref(d), L.stream()), "bd_ddpm_step")
    return (prev, x0) if want_x0 else prev


def ddim_step(model_output, sample, alphas_cumprod, t, prev_t, eta=0.0, noise=None, clip_sample=True,
              clip_sample_range=1.0, final_alpha_cumprod=1.0, out=None, want_x0=False, x0_quantile=None, sample_max_value=1.0):
    lib = L.load(); _need_cuda(model_output, sample, noise, alphas_cumprod)
    assert model_output.is_contiguous() and sample.is_contiguous()
    prev = torch.empty_like(sample) if out is None else out
    x0 = torch.empty_like(sample) if want_x0 else None
    d = L.DdimStepDesc(n=sample.numel(), model_output=L.ptr(model_output), sample=L.ptr(sample),
                       noise=L.ptr(noise.contiguous()) if noise is not None else None, prev_sample=L.ptr(prev),
                       pred_original=L.ptr(x0), alphas_cumprod=L.ptr(alphas_cumprod), t=int(t), prev_t=int(prev_t),
                       final_alpha_cumprod=final_alpha_cumprod, eta=eta, clip_sample=int(bool(clip_sample)),
                       clip_sample_range=clip_sample_range,
                       **_threshold_fields("ddim_step", sample, x0_quantile, sample_max_value))
    L.check(lib.bd_ddim_step(C.byref(d), L.stream()), "bd_ddim_step")
    return (prev, x0) if want_x0 else prev


def abs_quantile_plan(B, m):
    """bd_abs_quantile_plan as a dict: which path a (B, m) takes (path 0 registers, 1 stream), with how many workgroups and threads"""
    lib = L.load()
    info = L.AbsQuantilePlanInfo()
    L.check(lib.bd_abs_quantile_plan(int(B), int(m), C.byref(info)), "bd_abs_quantile_plan")
    return {name: getattr(info, name) for name, _ in info._fields_}


def abs_quantile(x, q, *, model_output=None, alphas_cumprod=None, t=None):
    """[B] float32: torch.quantile(|v|.reshape(B, -1), q, dim=1) bit for bit, raw (not clamped).  v = x, or with model_output
    (and the device table alphas_cumprod and the timestep t) the predicted x0 = (x - sqrt(1 - a_t) model_output) / sqrt(a_t), never
    materialised.  x (and model_output, in the same layout) is float32 and dense with dimension 0 outermost in memory: contiguous, or
    channels_last storage -- a quantile does not depend on the order inside an image."""
    lib = L.load(); _need_cuda(x, model_output, alphas_cumprod)
    if x.dtype != torch.float32 or x.dim() < 1 or x.numel() == 0:
        raise TypeError(f"abs_quantile: expected a non-empty float32 tensor, got {x.dtype} {tuple(x.shape)}")
    B = x.shape[0]
    m = x.numel() // B
    if not _is_dense(x) or (B > 1 and m > 1 and x.stride(0) != m):
        raise ValueError("abs_quantile: x must be dense with dimension 0 outermost in memory")
    if model_output is not None:
        if alphas_cumprod is None or t is None:
            raise ValueError("abs_quantile: model_output needs alphas_cumprod and t")
        if model_output.shape != x.shape or model_output.stride() != x.stride() or model_output.dtype != x.dtype \
                or model_output.device != x.device:
            raise ValueError("abs_quantile: x and model_output must share shape, strides, dtype and device")
        if alphas_cumprod.dtype != torch.float32 or not alphas_cumprod.is_contiguous():
            raise ValueError("abs_quantile: alphas_cumprod must be a contiguous float32 table")
    out = torch.empty(B, device=x.device, dtype=torch.float32)
    need = lib.bd_abs_quantile_workspace_bytes(B, m)
    ws = workspace(need, x.device, "abs_quantile") if need else None
    d = L.AbsQuantileDesc(B=B, m=m, x=L.ptr(x), model_output=L.ptr(model_output), alphas_cumprod=L.ptr(alphas_cumprod),
                          n_alphas=0 if alphas_cumprod is None else alphas_cumprod.numel(), t=0 if t is None else int(t), q=float(q),
                          out=L.ptr(out), workspace=L.ptr(ws), workspace_bytes=0 if ws is None else ws.numel())
    L.check(lib.bd_abs_quantile(C.byref(d), L.stream()), "bd_abs_quantile")
    return out


def _is_dense(t):
    """True when the tensor's elements fill one block of memory in some order of its dimensions"""
    expect = 1
    for d in sorted((d for d in range(t.dim()) if t.size(d) > 1), key=lambda d: t.stride(d)):
        if t.stride(d) != expect:
            return False
        expect *= t.size(d)
    return True


def _repaint_dense(who, ref, *others):
    """`ref` ([N,C,H,W] float32, made dense if it is not) and `others` brought to its strides: the dense operands of a RePaint kernel.
    A contiguous tensor next to NHWC storage goes through bd_nchw_to_nhwc; any other mismatch is a strided copy."""
    if ref.dim() != 4 or ref.dtype != torch.float32 or ref.numel() == 0:
        raise TypeError(f"{who}: expected a non-empty float32 [N,C,H,W] tensor, got {ref.dtype} {tuple(ref.shape)}")
    if not _is_dense(ref):
        ref = ref.contiguous()
    nhwc = ref.permute(0, 2, 3, 1).is_contiguous()
    out = [ref]
    for t in others:
        if t is None:
            out.append(None)
            continue
        if t.shape != ref.shape or t.dtype != torch.float32:
            raise ValueError(f"{who}: operands must all be float32 {tuple(ref.shape)}, got {t.dtype} {tuple(t.shape)}")
        if t.stride() != ref.stride():
            if nhwc and t.is_contiguous():
                t = nchw_to_nhwc(t).permute(0, 3, 1, 2)
            if t.stride() != ref.stride():
                t = torch.empty_like(ref).copy_(t)
        out.append(t)
    return out


def _repaint_bcast(who, name, t, shape):
    """a float32 operand broadcastable to `shape`, expanded by stride (0 along a broadcast dimension), never materialised"""
    if t.dtype != torch.float32:
        raise TypeError(f"{who}: {name} must be float32, got {t.dtype}")
    if t.dim() > 4:
        raise ValueError(f"{who}: {name} {tuple(t.shape)} does not broadcast to {tuple(shape)}")
    try:
        return t.reshape((1,) * (4 - t.dim()) + tuple(t.shape)).expand(*shape)
    except RuntimeError:
        raise ValueError(f"{who}: {name} {tuple(t.shape)} does not broadcast to {tuple(shape)}") from None


def repaint_step(model_output, sample, noise, original_image, mask, alphas_cumprod, t, prev_t, eta=0.0, clip_sample=True,
                 clip_sample_range=1.0, final_alpha_cumprod=1.0, shift=None, out=None, want_x0=False):
    """One RePaint reverse step (bd_repaint_step, formulas in include/bd_hip.h).  model_output / sample / noise: float32 [N,C,H,W] GPU
    tensors; the result has `sample`'s dense layout (NCHW, or a permuted view of NHWC storage).  original_image, mask and the optional
    shift broadcast to [N,C,H,W] and are read through their strides.  Returns prev_sample, or (prev_sample, pred_original_sample)."""
    lib = L.load(); _need_cuda(model_output, sample, noise, original_image, mask, alphas_cumprod, shift)
    sample, model_output, noise = _repaint_dense("repaint_step", sample, model_output, noise)
    N, Cc, H, W = sample.shape
    orig = _repaint_bcast("repaint_step", "original_image", original_image, sample.shape)
    msk = _repaint_bcast("repaint_step", "mask", mask, sample.shape)
    shf = None if shift is None else _repaint_bcast("repaint_step", "shift", shift, sample.shape)
    prev = torch.empty_like(sample) if out is None else out
    x0 = torch.empty_like(sample) if want_x0 else None
    if prev.stride() != sample.stride() or (x0 is not None and x0.stride() != sample.stride()):
        raise ValueError("repaint_step: out must have sample's strides")
    d = L.RepaintStepDesc(N=N, C=Cc, H=H, W=W, model_output=L.ptr(model_output), sample=L.ptr(sample), noise=L.ptr(noise),
                          prev_sample=L.ptr(prev), pred_original=L.ptr(x0), original_image=L.ptr(orig), mask=L.ptr(msk), shift=L.ptr(shf),
                          alphas_cumprod=L.ptr(alphas_cumprod), n_alphas=alphas_cumprod.numel(), t=int(t), prev_t=int(prev_t),
                          final_alpha_cumprod=final_alpha_cumprod, eta=eta, clip_sample=int(bool(clip_sample)),
                          clip_sample_range=clip_sample_range)
    for i in range(4):
        d.stride[i], d.orig_stride[i], d.mask_stride[i] = sample.stride(i), orig.stride(i), msk.stride(i)
        d.shift_stride[i] = 0 if shf is None else shf.stride(i)
    L.check(lib.bd_repaint_step(C.byref(d), L.stream()), "bd_repaint_step")
    return (prev, x0) if want_x0 else prev


def repaint_undo(sample, noises, betas, t, shift=None, out=None):
    """k = len(noises) forward sub-steps of RePaint's undo_step from timestep t (bd_repaint_undo): x <- sqrt(1 - betas[t+i]) x +
    sqrt(betas[t+i]) noises[i] [+ (1 - sqrt(1 - betas[t+i])) shift], in order.  sample and every noise: float32 [N,C,H,W] GPU tensors;
    the result has `sample`'s dense layout.  Any k >= 1: the library cuts it into launches of REPAINT_UNDO_MAX sub-steps."""
    lib = L.load(); _need_cuda(sample, betas, shift, *noises)
    k = len(noises)
    if k < 1:
        raise ValueError("repaint_undo: at least one noise tensor")
    sample, *noises = _repaint_dense("repaint_undo", sample, *noises)
    N, Cc, H, W = sample.shape
    shf = None if shift is None else _repaint_bcast("repaint_undo", "shift", shift, sample.shape)
    if out is None:
        out = torch.empty_like(sample)
    elif out.stride() != sample.stride():
        raise ValueError("repaint_undo: out must have sample's strides")
    d = L.RepaintUndoDesc(N=N, C=Cc, H=H, W=W, sample=L.ptr(sample), out=L.ptr(out), shift=L.ptr(shf), betas=L.ptr(betas),
                          n_betas=betas.numel(), t=int(t), k=k)
    for i in range(4):
        d.stride[i] = sample.stride(i)
        d.shift_stride[i] = 0 if shf is None else shf.stride(i)
    ptrs = (C.c_void_p * k)(*[z.data_ptr() for z in noises])
    L.check(lib.bd_repaint_undo(C.byref(d), ptrs, L.stream()), "bd_repaint_undo")
    return out


def to_image(x, nhwc, shape_bchw, want_u8=False):
    """(x/2+0.5).clamp(0,1) -> NHWC float32 [B,H,W,C] (and uint8 round(255 x))."""
    lib = L.load(); _need_cuda(x)
    B, Cc, H, W = shape_bchw
    x = x.contiguous()
    of = torch.empty(B, H, W, Cc, device=x.device)
    ou = torch.empty(B, H, W, Cc, dtype=torch.uint8, device=x.device) if want_u8 else None
    L.check(lib.bd_to_image(L.ptr(x), int(nhwc), Cc, B, Cc, H, W, L.ptr(of), L.ptr(ou), L.stream()), "bd_to_image")
    return (of, ou) if want_u8 else of


def timestep_embedding(t, dim, flip_sin_to_cos, freq_shift):
    lib = L.load(); _need_cuda(t)
    if t.is_floating_point():       # fractional timesteps: one rounding to fp32, as the reference's .float()
        t = t.float().contiguous()
        out = torch.empty(t.numel(), dim, device=t.device)
        L.check(lib.bd_timestep_embedding_f32(L.ptr(t), 1, t.numel(), dim, int(flip_sin_to_cos), float(freq_shift), L.ptr(out),
                                              L.stream()), "bd_timestep_embedding_f32")
        return out
    t = t.to(torch.int64).contiguous()
    out = torch.empty(t.numel(), dim, device=t.device)
    L.check(lib.bd_timestep_embedding(L.ptr(t), 1, t.numel(), dim, int(flip_sin_to_cos), float(freq_shift), L.ptr(out),
                                      L.stream()), "bd_timestep_embedding")
    return out


# ------------------------------------------------------------------------------------------------ GroupNorm
def gn_fwd(x, gamma, beta, G, eps, silu):
    """x [B,HW,C] (last dim contiguous, row stride = ld).  Returns (y [B,HW,C], mean [B,G], rstd [B,G])."""
    lib = L.load(); _need_cuda(x, gamma, beta)
    B, HW, Cc = x.shape
    y = torch.empty(B, HW, Cc, device=x.device)
    stats = torch.empty(2, B, G, device=x.device)
    ws = workspace(lib.bd_gn_workspace_bytes(B, Cc), x.device)
    d = L.GnFwdDesc(B=B, HW=HW, C=Cc, G=G, eps=eps, silu=int(silu), x=L.ptr(x), ldx=_ld(x), gamma=L.ptr(gamma),
                    beta=L.ptr(beta), y=L.ptr(y), ldy=Cc, mean=L.ptr(stats[0]), rstd=L.ptr(stats[1]),
                    workspace=L.ptr(ws), workspace_bytes=ws.numel())
    L.check(lib.bd_gn_fwd(C.byref(d), L.stream()), "bd_gn_fwd")
    return y, stats[0], stats[1]


def gn_bwd(x, gamma, beta, mean, rstd, dy, G, silu, dx=None, accumulate=False, with_colsum=False):
    """Returns (dx, dgamma, dbeta) and, with_colsum, the per-sample sum over pixels of dx [B, C]."""
    lib = L.load(); _need_cuda(x, gamma, beta, mean, rstd, dy)
    B, HW, Cc = x.shape
    if dx is None:
        dx = torch.empty(B, HW, Cc, device=x.device)
    dg = torch.empty(Cc, device=x.device); db = torch.empty(Cc, device=x.device)
    ws = workspace(lib.bd_gn_workspace_bytes(B, Cc), x.device)
    d = L.GnBwdDesc(B=B, HW=HW, C=Cc, G=G, silu=int(silu), x=L.ptr(x), ldx=_ld(x), gamma=L.ptr(gamma), beta=L.ptr(beta),
                    mean=L.ptr(mean), rstd=L.ptr(rstd), dy=L.ptr(dy), lddy=_ld(dy), dx=L.ptr(dx), lddx=_ld(dx),
                    accumulate_dx=int(accumulate), dgamma=L.ptr(dg), dbeta=L.ptr(db), workspace=L.ptr(ws),
                    workspace_bytes=ws.numel())
    cs = torch.empty(B, Cc, device=x.device) if with_colsum else None
    d.dx_colsum = L.ptr(cs); d.ld_colsum = Cc
    L.check(lib.bd_gn_bwd(C.byref(d), L.stream()), "bd_gn_bwd")
    return (dx, dg, db, cs) if with_colsum else (dx, dg, db)


# ------------------------------------------------------------------------------------------------ igemm family
def _conv_out_hw(Hs, Ws, stride, pad_t, pad_l, ups, pad_b=None, pad_r=None):
    Hi, Wi = Hs << ups, Ws << ups
    pad_b = pad_t if pad_b is None else pad_b
    pad_r = pad_l if pad_r is None else pad_r
    return (Hi + pad_t + pad_b - 3) // stride + 1, (Wi + pad_l + pad_r - 3) // stride + 1


def conv3x3_fwd(x, w, bias=None, stride=1, pad=1, ups=0, asym=False, rowbias=None, residual=None, out_scale=1.0, mode=0,
                w_split=None):
    """x [B,Hs,Ws,Cin] NHWC ; w [Cout,3,3,Cin].  asym => F.pad(0,1,0,1) + stride-2 conv with padding 0."""
    lib = L.load(); _need_cuda(x, w, bias, rowbias, residual)
    B, Hs, Ws, Cin = x.shape
    Cout = w.shape[0]
    pt = pl = 0 if asym else pad
    Ho, Wo = _conv_out_hw(Hs, Ws, stride, pt, pl, ups, 1 if asym else None, 1 if asym else None)
    y = torch.empty(B, Ho, Wo, Cout, device=x.device)
    ws = workspace(lib.bd_conv3x3_workspace_bytes(B, Ho, Wo, Hs, Ws, Cin, Cout, ups), x.device)
    d = L.ConvFwdDesc(B=B, Hs=Hs, Ws=Ws, Cin=Cin, Cout=Cout, stride=stride, pad_t=pt, pad_l=pl, ups=ups, Ho=Ho, Wo=Wo,
                      x=L.ptr(x), ldx=_ld(x), w=L.ptr(w), bias=L.ptr(bias), rowbias=L.ptr(rowbias),
                      ld_rowbias=rowbias.stride(0) if rowbias is not None else 0, residual=L.ptr(residual),
                      ldr=_ld(residual) if residual is not None else 0, out_scale=out_scale, y=L.ptr(y), ldy=Cout,
                      workspace=L.ptr(ws), workspace_bytes=ws.numel(), mode=mode)
    if w_split is not None:   # w already split (split_bf16): the weight operand is staged without VALU work
        d.w_split = L.ptr(w_split)
    L.check(lib.bd_conv3x3_fwd(C.byref(d), L.stream()), "bd_conv3x3_fwd")
    return y


def split_bf16(x):
    """The bf16 hi/lo split the bf16x3 kernels apply on the fly, as one int16 tensor [numel/32, 2, 32]
    (block, hi|lo, element): include/bd_hip.h bd_split_bf16."""
    lib = L.load(); _need_cuda(x)
    x = x.contiguous()
    out = torch.empty(x.numel() // 32, 2, 32, dtype=torch.int16, device=x.device)
    L.check(lib.bd_split_bf16(L.ptr(x), x.numel(), L.ptr(out), L.stream()), "bd_split_bf16")
    return out


def split_rows(x, out=None):
    """fp32 [..., C] (last dim contiguous, uniform row stride) -> split planes int16 [rows, C/32, 2, 32]
    (row, 32-channel block, hi|lo, element): include/bd_hip.h bd_split_rows."""
    lib = L.load(); _need_cuda(x)
    Cc = x.shape[-1]
    rows = x.numel() // Cc
    if out is None:
        out = torch.empty(rows, Cc // 32, 2, 32, dtype=torch.int16, device=x.device)
    L.check(lib.bd_split_rows(L.ptr(x), _ld(x), rows, Cc, L.ptr(out), Cc, L.stream()), "bd_split_rows")
    return out


def split_rows_ups2(x):
    """x [B,H,W,C] fp32 -> split planes of the nearest x2 upsampling, int16 [B*2H*2W, C/32, 2, 32]."""
    lib = L.load(); _need_cuda(x)
    B, H, W, Cc = x.shape
    out = torch.empty(B * 4 * H * W, Cc // 32, 2, 32, dtype=torch.int16, device=x.device)
    L.check(lib.bd_split_rows_ups2(L.ptr(x), _ld(x), B, H, W, Cc, L.ptr(out), Cc, L.stream()), "bd_split_rows_ups2")
    return out


def split_wT(w):
    """conv weight [Cout,3,3,Cin] fp32 -> split planes of the transpose [Cin,3,3,Cout] (for the data gradient)."""
    lib = L.load(); _need_cuda(w)
    Cout, _, _, Cin = w.shape
    out = torch.empty(Cin, 9 * Cout // 32, 2, 32, dtype=torch.int16, device=w.device)
    L.check(lib.bd_split_wt(L.ptr(w.contiguous()), Cin, Cout, L.ptr(out), L.stream()), "bd_split_wt")
    return out


def conv3x3_ps(x_split, w_split, B, H, W, K, N, direction=1, bias=None, rowbias=None, residual=None, out_scale=1.0,
               out=None, accumulate=False, gn_groups=0, mode=0):
    """stride-1 pad-1 3x3 convolution (direction +1) / data gradient (-1) on pre-split operands -> fp32 [B,H,W,N].
    mode (every split-plane wrapper): 0 / 1 = BD_MODE_BF16X3 (hi*hi + hi*lo + lo*hi), 2 = BD_MODE_BF16 (hi*hi, single pass).
    gn_groups > 0: also the GroupNorm partials of y from the epilogue -> (y, partials [B, S, gn_groups, 2] fp64), S =
    bd_conv3x3_ps_gn_splits() (raises when the call cannot produce them)."""
    lib = L.load(); _need_cuda(x_split, w_split, bias, rowbias, residual)
    y = torch.empty(B, H, W, N, device=x_split.device) if out is None else out
    part = None
    if gn_groups:
        S = lib.bd_conv3x3_ps_gn_splits(B, H, W, K, N, gn_groups)
        if S <= 0:
            raise ValueError("conv3x3_ps: this call cannot write GroupNorm partials (bd_conv3x3_ps_gn_splits() == 0)")
        part = torch.full((B, S, gn_groups, 2), float("nan"), dtype=torch.float64, device=x_split.device)
    d = L.ConvPsDesc(B=B, H=H, W=W, K=K, N=N, direction=direction, x_split=L.ptr(x_split), ldx=K, w_split=L.ptr(w_split),
                     bias=L.ptr(bias), rowbias=L.ptr(rowbias), ld_rowbias=rowbias.stride(0) if rowbias is not None else 0,
                     residual=L.ptr(residual), ldr=_ld(residual) if residual is not None else 0, out_scale=out_scale,
                     y=L.ptr(y), ldy=_ld(y), accumulate=int(accumulate), mode=mode)
    ws = workspace(lib.bd_conv3x3_ps_workspace_bytes(C.byref(d)), x_split.device, "ps")
    d.workspace = L.ptr(ws); d.workspace_bytes = ws.numel()
    if part is not None:
        d.gn_part = L.ptr(part); d.gn_groups = gn_groups
    L.check(lib.bd_conv3x3_ps(C.byref(d), L.stream()), "bd_conv3x3_ps")
    return y if part is None else (y, part)


def _plan_dict(info):
    return {name: v.decode() if isinstance(v, bytes) else v for name, v in ((n, getattr(info, n)) for n, _ in info._fields_)}


def conv3x3_ps_plan(B, H, W, K, N, direction=1, gn_groups=0, mode=0, epi=0):
    """bd_conv3x3_ps_plan of a dense call (ldx = K, ldy = N) as a dict: kernel (L.PS_*), tiles, K split, ring depth, grid, workspace bytes,
    profiler class, GroupNorm splits for gn_groups.  epi: bit 1 = residual, 2 = row bias, 4 = accumulate.  Host only, nothing is launched;
    raises what bd_conv3x3_ps would answer for a shape it refuses."""
    lib = L.load()
    d = L.ConvPsDesc(B=B, H=H, W=W, K=K, N=N, direction=direction, ldx=K, ldy=N, residual=16 if epi & 1 else None, ldr=N,
                     rowbias=16 if epi & 2 else None, ld_rowbias=N, accumulate=int(bool(epi & 4)), gn_groups=gn_groups, mode=mode)
    info = L.ConvPsPlanInfo()
    L.check(lib.bd_conv3x3_ps_plan(C.byref(d), C.byref(info)), "bd_conv3x3_ps_plan")
    return _plan_dict(info)


def conv3x3_ps_wgrad_plan(B, H, W, Cin, Cout, mode=0, phase=False):
    """bd_conv3x3_ps_wgrad_plan (phase: bd_upsample_conv_wgrad_plan, H x W the SOURCE grid) of a dense call as a dict: kernel (L.PS_WGRAD*),
    taps, tiles, slots, K split, slab layout, workspace bytes, profiler class.  Host only, nothing is launched."""
    lib = L.load()
    info = L.ConvPsWgradPlanInfo()
    if phase:
        d = L.UpsampleConvDesc(B=B, H=H, W=W, Cin=Cin, Cout=Cout, ldx=Cin, lddy=Cout, mode=mode)
        L.check(lib.bd_upsample_conv_wgrad_plan(C.byref(d), C.byref(info)), "bd_upsample_conv_wgrad_plan")
    else:
        d = L.ConvPsWgradDesc(B=B, H=H, W=W, Cin=Cin, Cout=Cout, ldx=Cin, lddy=Cout, mode=mode)
        L.check(lib.bd_conv3x3_ps_wgrad_plan(C.byref(d), C.byref(info)), "bd_conv3x3_ps_wgrad_plan")
    return _plan_dict(info)


def conv3x3_ps_wgrad(x_split, dy_split, B, H, W, Cin, Cout, with_db=False, mode=0):
    """dw [Cout,3,3,Cin] (and db [Cout]) of the stride-1 pad-1 conv from split-plane operands."""
    lib = L.load(); _need_cuda(x_split, dy_split)
    dw = torch.empty(Cout, 3, 3, Cin, device=x_split.device)
    db = torch.empty(Cout, device=x_split.device) if with_db else None
    d = L.ConvPsWgradDesc(B=B, H=H, W=W, Cin=Cin, Cout=Cout, x_split=L.ptr(x_split), ldx=Cin, dy_split=L.ptr(dy_split),
                          lddy=Cout, dw=L.ptr(dw), db=L.ptr(db), mode=mode)
    ws = workspace(lib.bd_conv3x3_ps_wgrad_workspace_bytes(C.byref(d)), x_split.device, "ps_wgrad")
    d.workspace = L.ptr(ws); d.workspace_bytes = ws.numel()
    L.check(lib.bd_conv3x3_ps_wgrad(C.byref(d), L.stream()), "bd_conv3x3_ps_wgrad")
    return (dw, db) if with_db else dw


def upsample_weights(w):
    """conv weight [Cout,3,3,Cin] of an Upsample2D layer -> (E planes [Cout,16,Cin], E^T planes [Cin,16,Cout]) as split planes:
    E[oy][ox] = sum of the taps that read the same source pixel (include/bd_hip.h, phase-decomposed convolutions)."""
    lib = L.load(); _need_cuda(w)
    Cout, _, _, Cin = w.shape
    e = torch.empty(Cout, 16 * Cin // 32, 2, 32, dtype=torch.int16, device=w.device)
    et = torch.empty(Cin, 16 * Cout // 32, 2, 32, dtype=torch.int16, device=w.device)
    L.check(lib.bd_upsample_weights(L.ptr(w.contiguous()), Cin, Cout, L.ptr(e), L.ptr(et), L.stream()), "bd_upsample_weights")
    return e, et


def upsample_conv_fwd(x_split, e_split, B, H, W, Cin, Cout, bias=None, mode=0):
    """y [B,2H,2W,Cout] = conv3x3(nearest_up2(x)) + bias from the SOURCE-grid split planes of x and the E planes."""
    lib = L.load(); _need_cuda(x_split, e_split, bias)
    y = torch.empty(B, 2 * H, 2 * W, Cout, device=x_split.device)
    d = L.UpsampleConvDesc(B=B, H=H, W=W, Cin=Cin, Cout=Cout, x_split=L.ptr(x_split), ldx=Cin, e_split=L.ptr(e_split), bias=L.ptr(bias),
                           y=L.ptr(y), ldy=Cout, mode=mode)
    L.check(lib.bd_upsample_conv_fwd(C.byref(d), L.stream()), "bd_upsample_conv_fwd")
    return y


def upsample_conv_dgrad(dy_split, et_split, B, H, W, Cin, Cout, out=None, accumulate=False, mode=0):
    """dx [B,H,W,Cin] of the same layer from the fine-grid split planes of dY [B,2H,2W,Cout] and the E^T planes."""
    lib = L.load(); _need_cuda(dy_split, et_split)
    dx = torch.empty(B, H, W, Cin, device=dy_split.device) if out is None else out
    d = L.UpsampleConvDesc(B=B, H=H, W=W, Cin=Cin, Cout=Cout, dy_split=L.ptr(dy_split), lddy=Cout, et_split=L.ptr(et_split),
                           dx=L.ptr(dx), lddx=_ld(dx), accumulate=int(accumulate), mode=mode)
    ws = workspace(lib.bd_upsample_conv_dgrad_workspace_bytes(C.byref(d)), dy_split.device, "ups_dgrad")
    d.workspace = L.ptr(ws); d.workspace_bytes = ws.numel()
    L.check(lib.bd_upsample_conv_dgrad(C.byref(d), L.stream()), "bd_upsample_conv_dgrad")
    return dx


def upsample_conv_wgrad(x_split, dy_split, B, H, W, Cin, Cout, with_db=False, mode=0):
    """dw [Cout,3,3,Cin] (and db) of the same layer from x (source grid) and dY (fine grid), both split planes."""
    lib = L.load(); _need_cuda(x_split, dy_split)
    dw = torch.empty(Cout, 3, 3, Cin, device=x_split.device)
    db = torch.empty(Cout, device=x_split.device) if with_db else None
    d = L.UpsampleConvDesc(B=B, H=H, W=W, Cin=Cin, Cout=Cout, x_split=L.ptr(x_split), ldx=Cin, dy_split=L.ptr(dy_split), lddy=Cout,
                           dw=L.ptr(dw), db=L.ptr(db), mode=mode)
    ws = workspace(lib.bd_upsample_conv_wgrad_workspace_bytes(C.byref(d)), x_split.device, "ups_wgrad")
    d.workspace = L.ptr(ws); d.workspace_bytes = ws.numel()
    L.check(lib.bd_upsample_conv_wgrad(C.byref(d), L.stream()), "bd_upsample_conv_wgrad")
    return (dw, db) if with_db else dw


def conv3x3_s2_dgrad_ps(dy_split, wT_split, B, Ho, Wo, Cin, Cout, pad=0, out=None, accumulate=False, mode=0):
    """dx [B,2Ho,2Wo,Cin] of a stride-2 3x3 convolution (pad 0 = F.pad(0,1,0,1) + padding 0; 1 = padding 1) from the split planes
    of dy [B,Ho,Wo,Cout] and the transposed weight planes (split_wT)."""
    lib = L.load(); _need_cuda(dy_split, wT_split)
    dx = torch.empty(B, 2 * Ho, 2 * Wo, Cin, device=dy_split.device) if out is None else out
    d = L.ConvS2DgradDesc(B=B, Ho=Ho, Wo=Wo, Cin=Cin, Cout=Cout, pad=pad, dy_split=L.ptr(dy_split), lddy=Cout, wT_split=L.ptr(wT_split),
                          dx=L.ptr(dx), lddx=_ld(dx), accumulate=int(accumulate), mode=mode)
    L.check(lib.bd_conv3x3_s2_dgrad_ps(C.byref(d), L.stream()), "bd_conv3x3_s2_dgrad_ps")
    return dx


def conv3x3_dgrad(dy, w, x_shape, stride=1, pad=1, ups=0, asym=False, mode=0, w_split=None):
    """Returns dx over the conv's own input grid [B, Hs<<ups, Ws<<ups, Cin]."""
    lib = L.load(); _need_cuda(dy, w)
    B, Hs, Ws, Cin = x_shape
    Cout = w.shape[0]
    pt = pl = 0 if asym else pad
    Ho, Wo = dy.shape[1], dy.shape[2]
    dx = torch.empty(B, Hs << ups, Ws << ups, Cin, device=dy.device)
    ws = workspace(lib.bd_conv3x3_workspace_bytes(B, Ho, Wo, Hs, Ws, Cin, Cout, ups), dy.device)
    d = L.ConvDgradDesc(B=B, Hs=Hs, Ws=Ws, Cin=Cin, Cout=Cout, stride=stride, pad_t=pt, pad_l=pl, ups=ups, Ho=Ho, Wo=Wo,
                        dy=L.ptr(dy), lddy=_ld(dy), w=L.ptr(w), dx=L.ptr(dx), lddx=Cin, accumulate=0,
                        workspace=L.ptr(ws), workspace_bytes=ws.numel(), mode=mode)
    if w_split is not None:
        d.w_split = L.ptr(w_split)
    L.check(lib.bd_conv3x3_dgrad(C.byref(d), L.stream()), "bd_conv3x3_dgrad")
    return dx


def conv3x3_wgrad(x, dy, stride=1, pad=1, ups=0, asym=False, mode=0, with_db=False):
    """dw [Cout,3,3,Cin]; with_db also returns the bias gradient (sum of dy over pixels) fused into the same launch."""
    lib = L.load(); _need_cuda(x, dy)
    B, Hs, Ws, Cin = x.shape
    Cout = dy.shape[-1]
    pt = pl = 0 if asym else pad
    Ho, Wo = dy.shape[1], dy.shape[2]
    dw = torch.empty(Cout, 3, 3, Cin, device=x.device)
    ws = workspace(lib.bd_conv3x3_workspace_bytes(B, Ho, Wo, Hs, Ws, Cin, Cout, ups), x.device)
    d = L.ConvWgradDesc(B=B, Hs=Hs, Ws=Ws, Cin=Cin, Cout=Cout, stride=stride, pad_t=pt, pad_l=pl, ups=ups, Ho=Ho, Wo=Wo,
                        x=L.ptr(x), ldx=_ld(x), dy=L.ptr(dy), lddy=_ld(dy), dw=L.ptr(dw), workspace=L.ptr(ws),
                        workspace_bytes=ws.numel(), mode=mode)
    db = torch.empty(Cout, device=x.device) if with_db else None
    d.db = L.ptr(db)
    L.check(lib.bd_conv3x3_wgrad(C.byref(d), L.stream()), "bd_conv3x3_wgrad")
    return (dw, db) if with_db else dw


def gemm(a, b, trans_a=False, trans_b=True, bias=None, alpha=1.0, tile=0, ksplit=0, mode=0, a_colsum=None):
    """C = alpha * op(a) @ op(b)^T-style product on the igemm engine.
    a: [M,K] (trans_a False) or [K,M] (trans_a True); b: [N,K] (trans_b True, 'weights') or [K,N] (False).
    Batched when a/b are 3-D (same leading batch)."""
    lib = L.load(); _need_cuda(a, b, bias)
    batched = a.dim() == 3
    if not batched:
        a, b = a[None], b[None]
    nb = a.shape[0]
    M, K = (a.shape[2], a.shape[1]) if trans_a else (a.shape[1], a.shape[2])
    N = b.shape[1] if trans_b else b.shape[2]
    a = a.contiguous(); b = b.contiguous()
    c = torch.empty(nb, M, N, device=a.device)
    d = L.IgemmDesc()
    d.A.kind = 0; d.A.kc = 0 if trans_a else 1; d.A.p = L.ptr(a); d.A.ld = a.shape[2]; d.A.bs_outer = a.stride(0)
    d.B.kind = 0; d.B.kc = 1 if trans_b else 0; d.B.p = L.ptr(b); d.B.ld = b.shape[2]; d.B.bs_outer = b.stride(0)
    d.M, d.N, d.K = M, N, K
    d.batch_outer, d.batch_inner = nb, 1
    d.C = L.ptr(c); d.ldc = N; d.c_bs_outer = M * N
    d.alpha = alpha; d.out_scale = 1.0; d.bias = L.ptr(bias)
    d.tile = tile; d.ksplit = ksplit; d.mode = mode; d.a_colsum = L.ptr(a_colsum)
    need = lib.bd_igemm_workspace_bytes(C.byref(d))
    ws = workspace(need, a.device)
    d.workspace = L.ptr(ws); d.workspace_bytes = ws.numel()
    L.check(lib.bd_igemm(C.byref(d), L.stream()), "bd_igemm")
    return c if batched else c[0]


def unsplit_rows(s):
    """Split planes int16 [..., C/32, 2, 32] -> fp32 [..., C] (hi + lo, exact): test / inspection helper, plain torch."""
    hi = (s[..., 0, :].to(torch.int32) << 16).view(torch.float32)
    lo = (s[..., 1, :].to(torch.int32) << 16).view(torch.float32)
    return (hi + lo).reshape(*s.shape[:-3], s.shape[-3] * 32)


def gemm_sp(a_split, b_split, M, N, K, a_kmajor=False, b_kmajor=False, batch=1, bias=None, residual=None, alpha=1.0, out_scale=1.0,
            want_f32=True, want_split=False, out=None, accumulate=False, want_colsum=False, mode=0):
    """C = out_scale * (alpha * A B^T + bias + residual) on split planes (include/bd_hip.h bd_gemm_sp).  a_split: planes of A [batch, M, K]
    (or [batch, K, M] when a_kmajor); b_split: planes of B [batch, N, K] (or [batch, K, N] when b_kmajor), or un-batched (shared by the
    batch).  Returns (c fp32 or None, c_split or None[, colsum])."""
    lib = L.load(); _need_cuda(a_split, b_split, bias, residual)
    dev = a_split.device
    d = L.GemmSpDesc()
    d.M, d.N, d.K, d.batch, d.mode = M, N, K, batch, mode
    ar, ac = (K, M) if a_kmajor else (M, K)
    br, bc = (K, N) if b_kmajor else (N, K)
    d.a = L.ptr(a_split); d.lda = ac; d.a_bs = ar * ac if a_split.numel() * 2 == batch * ar * ac * 4 else 0; d.a_kmajor = int(a_kmajor)
    d.b = L.ptr(b_split); d.ldb = bc; d.b_bs = br * bc if b_split.numel() * 2 == batch * br * bc * 4 else 0; d.b_kmajor = int(b_kmajor)
    c = out if out is not None else (torch.empty(batch, M, N, device=dev) if want_f32 else None)
    cs = torch.empty(batch, M, N // 32, 2, 32, dtype=torch.int16, device=dev) if want_split else None
    d.c = L.ptr(c); d.ldc = N; d.c_bs = M * N
    d.c_split = L.ptr(cs); d.ldcs = N; d.cs_bs = M * N
    d.bias = L.ptr(bias)
    if residual is not None:
        residual = residual.contiguous()
        d.residual = L.ptr(residual); d.ldr = N; d.r_bs = M * N
    d.alpha = alpha; d.out_scale = out_scale; d.accumulate = int(accumulate)
    colsum_t = torch.empty(M, device=dev) if want_colsum else None
    d.a_colsum = L.ptr(colsum_t)
    need = lib.bd_gemm_sp_workspace_bytes(C.byref(d))
    ws = workspace(need, dev)
    d.workspace = L.ptr(ws); d.workspace_bytes = ws.numel()
    L.check(lib.bd_gemm_sp(C.byref(d), L.stream()), "bd_gemm_sp")
    return (c, cs, colsum_t) if want_colsum else (c, cs)


def gemm_sp_plan(M, N, K, batch=1, a_kmajor=False, b_kmajor=False, a_colsum=False, mode=0):
    """bd_gemm_sp_plan of a dense call with an fp32 output as a dict: operand form (2 * a_kmajor + b_kmajor), tiles, batch, K split, grid,
    second passes, workspace bytes, offset of the column-sum rows, profiler class.  Host only, nothing is launched; raises what bd_gemm_sp
    would answer for a shape it refuses."""
    lib = L.load()
    ar, ac = (K, M) if a_kmajor else (M, K)
    br, bc = (K, N) if b_kmajor else (N, K)
    d = L.GemmSpDesc(M=M, N=N, K=K, batch=batch, lda=ac, a_bs=ar * ac, a_kmajor=int(a_kmajor), ldb=bc, b_bs=br * bc, b_kmajor=int(b_kmajor),
                     c=16, ldc=N, c_bs=M * N, alpha=1.0, out_scale=1.0, a_colsum=16 if a_colsum else None, mode=mode)
    info = L.GemmSpPlanInfo()
    L.check(lib.bd_gemm_sp_plan(C.byref(d), C.byref(info)), "bd_gemm_sp_plan")
    return _plan_dict(info)


# ------------------------------------------------------------------------------------------------ small ops
def colsum(x, rows_per_group):
    lib = L.load(); _need_cuda(x)
    rows, N = x.shape
    groups = (rows + rows_per_group - 1) // rows_per_group
    out = torch.empty(groups, N, device=x.device)
    L.check(lib.bd_colsum(L.ptr(x), _ld(x), rows, N, rows_per_group, L.ptr(out), N, 0, L.stream()), "bd_colsum")
    return out


def sum2x2(du):
    lib = L.load(); _need_cuda(du)
    B, H2, W2, Cc = du.shape
    dx = torch.empty(B, H2 // 2, W2 // 2, Cc, device=du.device)
    L.check(lib.bd_sum2x2(L.ptr(du), Cc, L.ptr(dx), Cc, B, H2 // 2, W2 // 2, Cc, 0, L.stream()), "bd_sum2x2")
    return dx


def attn_sp_fwd(qkv_split, B, heads, scale, want_pt=True, C_=None, mode=0):
    """Attention core forward on the planes of the QKV projection's output [B*N, 3C/32, 2, 32] (include/bd_hip.h bd_attn_sp_fwd):
    returns (o_split [B*N, C/32, 2, 32], pt_split [B*heads, N, N/32, 2, 32] or None)."""
    lib = L.load(); _need_cuda(qkv_split)
    rows, blocks = qkv_split.shape[0], qkv_split.shape[1]
    N = rows // B
    Cc = C_ or blocks * 32 // 3            # C_: the planes' rows are padded beyond 3C (row stride = blocks * 32)
    o = torch.empty(rows, Cc // 32, 2, 32, dtype=torch.int16, device=qkv_split.device)
    pt = torch.empty(B * heads, N, N // 32, 2, 32, dtype=torch.int16, device=qkv_split.device) if want_pt else None
    d = L.AttnSpDesc(B=B, heads=heads, N=N, dh=Cc // heads, qkv_split=L.ptr(qkv_split), ld=blocks * 32, scale=scale, o_split=L.ptr(o), ldo=Cc,
                     pt_split=L.ptr(pt), mode=mode)
    L.check(lib.bd_attn_sp_fwd(C.byref(d), L.stream()), "bd_attn_sp_fwd")
    return o, pt


def attn_sp_bwd(qkv_split, pt_split, do_split, B, heads, scale, mode=0):
    """Attention core backward: returns (dqkv_split [B*N, 3C/32, 2, 32], dst_split = planes of scale * dS^T)."""
    lib = L.load(); _need_cuda(qkv_split, pt_split, do_split)
    rows, blocks = qkv_split.shape[0], qkv_split.shape[1]
    N = rows // B
    Cc = blocks * 32 // 3
    dqkv = torch.empty_like(qkv_split)
    dst = torch.empty_like(pt_split)
    d = L.AttnSpDesc(B=B, heads=heads, N=N, dh=Cc // heads, qkv_split=L.ptr(qkv_split), ld=3 * Cc, scale=scale, pt_split=L.ptr(pt_split),
                     do_split=L.ptr(do_split), lddo=Cc, dst_split=L.ptr(dst), dqkv_split=L.ptr(dqkv), lddqkv=3 * Cc, mode=mode)
    L.check(lib.bd_attn_sp_bwd(C.byref(d), L.stream()), "bd_attn_sp_bwd")
    return dqkv, dst


def softmax_fwd(s):
    lib = L.load(); _need_cuda(s)
    s = s.contiguous()
    p = torch.empty_like(s)
    L.check(lib.bd_softmax_fwd(L.ptr(s), L.ptr(p), s.numel() // s.shape[-1], s.shape[-1], L.stream()), "bd_softmax_fwd")
    return p


def softmax_bwd(p, dp):
    lib = L.load(); _need_cuda(p, dp)
    ds = torch.empty_like(p)
    L.check(lib.bd_softmax_bwd(L.ptr(p.contiguous()), L.ptr(dp.contiguous()), L.ptr(ds), p.numel() // p.shape[-1],
                               p.shape[-1], L.stream()), "bd_softmax_bwd")
    return ds


def silu_fwd(x):
    lib = L.load(); _need_cuda(x)
    y = torch.empty_like(x)
    L.check(lib.bd_silu_fwd(L.ptr(x.contiguous()), L.ptr(y), x.numel(), L.stream()), "bd_silu_fwd")
    return y


def silu_bwd(x, dy):
    lib = L.load(); _need_cuda(x, dy)
    dx = torch.empty_like(x)
    L.check(lib.bd_silu_bwd(L.ptr(x.contiguous()), L.ptr(dy.contiguous()), L.ptr(dx), x.numel(), 0, L.stream()), "bd_silu_bwd")
    return dx


LOSS_TYPES = {"l2": 0, "l1": 1, "huber": 2}


def loss_fwd_bwd(pred, target, loss_type="l2", grad_scale=1.0, want_grad=True):
    """pred / target: [..., C] views with the same logical shape (last dim contiguous, uniform row stride).
    Returns (loss 0-dim tensor, dpred contiguous [rows, C] or None)."""
    lib = L.load(); _need_cuda(pred, target)
    if loss_type not in LOSS_TYPES:
        raise NotImplementedError()
    Cc = pred.shape[-1]
    rows = pred.numel() // Cc
    p2 = pred.reshape(rows, Cc) if pred.is_contiguous() else pred
    t2 = target.reshape(rows, Cc) if target.is_contiguous() else target
    loss = torch.empty((), device=pred.device)
    dp = torch.empty(rows, Cc, device=pred.device) if want_grad else None
    ws = workspace(lib.bd_reduce_workspace_bytes(), pred.device, "reduce")
    L.check(lib.bd_loss_fwd_bwd(L.ptr(p2), _ld(p2), L.ptr(t2), _ld(t2), rows, Cc, LOSS_TYPES[loss_type], grad_scale,
                                L.ptr(loss), L.ptr(dp), Cc, L.ptr(ws), L.stream()), "bd_loss_fwd_bwd")
    return loss, dp


def loss_groups_fwd_bwd(pred, target, groups, loss_type="l2", grad_scale=1.0, want_grad=True):
    """The loss of loss_fwd_bwd over consecutive groups of rows (bd_loss_groups_fwd_bwd).  pred / target as in loss_fwd_bwd; `groups` is a
    sequence of (row_count, weight) in rows of the [rows, C] view, 1 .. 4 of them, counts > 0 summing to rows, weights finite and >= 0.
    Returns (losses float [n_groups + 1]: each group's own mean, then sum_g weight_g * mean_g; dpred contiguous [rows, C] or None),
    dpred = d(weighted total)/dpred * grad_scale."""
    lib = L.load(); _need_cuda(pred, target)
    if loss_type not in LOSS_TYPES:
        raise NotImplementedError()
    groups = [(int(r), float(w)) for r, w in groups]
    if not 1 <= len(groups) <= L.LOSS_MAX_GROUPS:
        raise ValueError(f"loss_groups_fwd_bwd: 1..{L.LOSS_MAX_GROUPS} groups, got {len(groups)}")
    Cc = pred.shape[-1]
    rows = pred.numel() // Cc
    p2 = pred.reshape(rows, Cc) if pred.is_contiguous() else pred
    t2 = target.reshape(rows, Cc) if target.is_contiguous() else target
    d = L.LossGroupsDesc(n_groups=len(groups))
    for g, (r, w) in enumerate(groups):
        d.group_rows[g], d.group_weight[g] = r, w
    losses = torch.empty(len(groups) + 1, device=pred.device)
    dp = torch.empty(rows, Cc, device=pred.device) if want_grad else None
    nbytes = lib.bd_loss_groups_workspace_bytes(len(groups))
    ws = workspace(nbytes, pred.device, "reduce")
    L.check(lib.bd_loss_groups_fwd_bwd(L.ptr(p2), _ld(p2), L.ptr(t2), _ld(t2), rows, Cc, LOSS_TYPES[loss_type], grad_scale, C.byref(d),
                                       L.ptr(losses), L.ptr(dp), Cc, L.ptr(ws), ws.numel(), L.stream()), "bd_loss_groups_fwd_bwd")
    return losses, dp


def _dense_out(who, first, others, out):
    """What the wrappers of the dense vec4 kernels open with: `first` is non-empty, float32 and dense, and every tensor of `others`
    that is present, and `out`, has its shape, strides and dtype.  Returns out, allocated like `first` when None."""
    if first.dtype != torch.float32 or first.numel() == 0 or not _is_dense(first):
        raise ValueError(f"{who}: tensors must be non-empty, float32 and dense")
    if out is None:
        out = torch.empty_like(first)
    for t in (*others, out):
        if t is not None and (t.shape != first.shape or t.stride() != first.stride() or t.dtype != torch.float32):
            raise ValueError(f"{who}: tensors must share shape, strides and dtype float32")
    return out


def _clip_pair(clip):
    """None or the range of a clamp -> the descriptor's (flag, range)"""
    return (0, 0.0) if clip is None else (1, float(clip))


def lincomb(terms, coeffs, clip=None, out=None):
    """out = clamp?(sum_j coeffs[j] * terms[j]) (bd_lincomb): up to 6 dense float32 GPU tensors of one shape and layout.  out (of the
    terms' shape, strides and dtype) may be one of the terms; the library refuses any other overlap."""
    lib = L.load(); _need_cuda(*terms, out)
    k = len(terms)
    if k < 1 or k > 6 or len(coeffs) != k:
        raise ValueError("lincomb: 1..6 terms with one coefficient each")
    out = _dense_out("lincomb", terms[0], terms[1:], out)
    ptrs = (C.c_void_p * k)(*[t.data_ptr() for t in terms])
    cs = (C.c_float * k)(*[float(c) for c in coeffs])
    L.check(lib.bd_lincomb(k, ptrs, cs, terms[0].numel(), *_clip_pair(clip), L.ptr(out), L.stream()), "bd_lincomb")
    return out


def dpm_step(model_output, sample, cx, c0, m1=None, c1=0.0, m2=None, c2=0.0, convert=None, x0_clip=None, clip=None, m0_out=None,
             out=None):
    """One DPM-Solver(++) multistep update (bd_dpm_step, formula in include/bd_hip.h) over dense float32 GPU tensors of one shape and
    layout.  convert: None (m0 = model_output, dpmsolver) or (alpha_s, sigma_s) (m0 = (sample - sigma_s model_output) / alpha_s,
    dpmsolver++); x0_clip / clip: None or the range of the clamp of m0 / of the result; m1 / m2: the stored converted outputs of the
    previous two steps, or None (term absent); m0_out: where m0 is written, or None.  out may be `sample`, m0_out may be the oldest
    history buffer (m2 included): the library refuses any other overlap.  Returns prev_sample."""
    lib = L.load(); _need_cuda(model_output, sample, m1, m2, m0_out, out)
    out = _dense_out("dpm_step", sample, (model_output, m1, m2, m0_out), out)
    alpha_s, sigma_s = (1.0, 0.0) if convert is None else convert
    (x0_on, x0_range), (clip_on, clip_range) = _clip_pair(x0_clip), _clip_pair(clip)
    d = L.DpmStepDesc(n=sample.numel(), model_output=L.ptr(model_output), sample=L.ptr(sample), m1=L.ptr(m1), m2=L.ptr(m2),
                      m0_out=L.ptr(m0_out), prev_out=L.ptr(out), convert=int(convert is not None), alpha_s=float(alpha_s),
                      sigma_s=float(sigma_s), x0_clip=x0_on, x0_range=x0_range, cx=float(cx), c0=float(c0), c1=float(c1), c2=float(c2),
                      clip=clip_on, clip_range=clip_range)
    L.check(lib.bd_dpm_step(C.byref(d), L.stream()), "bd_dpm_step")
    return out


def unipc_step(model_output, sample, px, p0, h1=None, p1=0.0, h2=None, p2=0.0, h3=None, last_sample=None, kl=0.0, k0=0.0, k1=0.0, k2=0.0,
               k3=0.0, convert=None, x0_clip=None, clip=None, m0_out=None, corrected_out=None, out=None):
    """One whole UniPC step (bd_unipc_step, formula in include/bd_hip.h) over dense float32 GPU tensors of one shape and layout:
    conversion, corrector, predictor.  convert / x0_clip / clip as in dpm_step; h1 / h2 / h3: the stored converted outputs of the
    previous steps, newest first, or None (term absent, its coefficients ignored); last_sample: the corrected sample of the previous
    step, or None (no corrector: the corrected sample is `sample`); m0_out / corrected_out: where m0 / the corrected sample are
    written, or None.  out may be `sample`, corrected_out may be `last_sample`, m0_out may be the oldest history buffer (h2 or h3
    included): the library refuses any other overlap.  Returns prev_sample."""
    lib = L.load(); _need_cuda(model_output, sample, last_sample, h1, h2, h3, m0_out, corrected_out, out)
    out = _dense_out("unipc_step", sample, (model_output, last_sample, h1, h2, h3, m0_out, corrected_out), out)
    alpha_s, sigma_s = (1.0, 0.0) if convert is None else convert
    (x0_on, x0_range), (clip_on, clip_range) = _clip_pair(x0_clip), _clip_pair(clip)
    d = L.UnipcStepDesc(n=sample.numel(), model_output=L.ptr(model_output), sample=L.ptr(sample), last_sample=L.ptr(last_sample),
                        h1=L.ptr(h1), h2=L.ptr(h2), h3=L.ptr(h3), m0_out=L.ptr(m0_out), corrected_out=L.ptr(corrected_out),
                        prev_out=L.ptr(out), convert=int(convert is not None), alpha_s=float(alpha_s), sigma_s=float(sigma_s),
                        x0_clip=x0_on, x0_range=x0_range, kl=float(kl), k0=float(k0), k1=float(k1), k2=float(k2), k3=float(k3),
                        px=float(px), p0=float(p0), p1=float(p1), p2=float(p2), clip=clip_on, clip_range=clip_range)
    L.check(lib.bd_unipc_step(C.byref(d), L.stream()), "bd_unipc_step")
    return out


def deis_step(model_output, sample, alpha_s, sigma_s, cx=0.0, c0=0.0, m1=None, alpha_t=0.0, k0=0.0, k1=0.0, m2=None, k2=0.0, x0_clip=None,
              clip=None, m0_out=None, out=None):
    """One DEIS multistep update (bd_deis_step, formula in include/bd_hip.h) over dense float32 GPU tensors of one shape and layout.
    (alpha_s, sigma_s): the scalars of the conversion m0 = (sample - alpha_s x0) / sigma_s, x0 = (sample - sigma_s model_output) /
    alpha_s; x0_clip / clip: None or the range of the clamp of x0 / of the result; m1 / m2: the stored converted outputs of the
    previous two steps, or None.  Without m1 the update is first order, cx sample - c0 m0; with it alpha_t (sample / alpha_s + k0 m0 +
    k1 m1 [+ k2 m2]).  m0_out: where m0 is written, or None.  out may be `sample`, m0_out may be the oldest history buffer (m2
    included): the library refuses any other overlap.  Returns prev_sample."""
    lib = L.load(); _need_cuda(model_output, sample, m1, m2, m0_out, out)
    out = _dense_out("deis_step", sample, (model_output, m1, m2, m0_out), out)
    (x0_on, x0_range), (clip_on, clip_range) = _clip_pair(x0_clip), _clip_pair(clip)
    d = L.DeisStepDesc(n=sample.numel(), model_output=L.ptr(model_output), sample=L.ptr(sample), m1=L.ptr(m1), m2=L.ptr(m2),
                       m0_out=L.ptr(m0_out), prev_out=L.ptr(out), alpha_s=float(alpha_s), sigma_s=float(sigma_s), x0_clip=x0_on,
                       x0_range=x0_range, cx=float(cx), c0=float(c0), alpha_t=float(alpha_t), k0=float(k0), k1=float(k1), k2=float(k2),
                       clip=clip_on, clip_range=clip_range)
    L.check(lib.bd_deis_step(C.byref(d), L.stream()), "bd_deis_step")
    return out


def sigma_step(model_output, sample, sigma_in, c0, in_div, base=None, average=False, h1=None, c1=0.0, h2=None, c2=0.0, h3=None, c3=0.0,
               clip=None, x0_out=None, d_out=None, scaled_out=None, out=None):
    """One transition of a sigma-space sampler (bd_sigma_step, formula in include/bd_hip.h) over dense float32 GPU tensors of one shape
    and layout: Euler (no history), Heun's averaging stage (average=True, h1 = the first stage's derivative, base = the sample that
    stage started from) or a linear multistep sum over h1..h3.  in_div = sqrt(sigma_next^2 + 1) scales the result into scaled_out, the
    next evaluation's model input; clip: None or the range of the clamp in those coordinates.  x0_out / d_out / scaled_out: where
    pred_original_sample, the derivative and the scaled sample are written, or None.  d_out may be the oldest history buffer, out may
    be `sample`: the library refuses any other overlap.  Returns prev_sample."""
    lib = L.load(); _need_cuda(model_output, sample, base, h1, h2, h3, x0_out, d_out, scaled_out, out)
    out = _dense_out("sigma_step", sample, (model_output, base, h1, h2, h3, x0_out, d_out, scaled_out), out)
    clip_on, clip_range = _clip_pair(clip)
    d = L.SigmaStepDesc(n=sample.numel(), model_output=L.ptr(model_output), sample=L.ptr(sample), base=L.ptr(base), h1=L.ptr(h1),
                        h2=L.ptr(h2), h3=L.ptr(h3), x0_out=L.ptr(x0_out), d_out=L.ptr(d_out), prev_out=L.ptr(out),
                        scaled_out=L.ptr(scaled_out), sigma_in=float(sigma_in), average=int(bool(average)), c0=float(c0), c1=float(c1),
                        c2=float(c2), c3=float(c3), in_div=float(in_div), clip=clip_on, clip_range=clip_range)
    L.check(lib.bd_sigma_step(C.byref(d), L.stream()), "bd_sigma_step")
    return out


def sigma_noise_step(model_output, sample, noise, sigma_in, dt, in_div, base=None, churn=None, sigma_up=None, clip=None, x0_out=None,
                     scaled_out=None, out=None):
    """One first order transition of a stochastic sigma-space sampler (bd_sigma_noise_step, formula in include/bd_hip.h) over dense
    float32 GPU tensors of one shape and layout.  churn: None or (s_noise, churn_mul), Euler's churn -- the sample is raised by
    (noise * s_noise) * churn_mul before anything reads it; sigma_up: None or the factor of the ancestral noise added to the updated
    sample (0.0 is a value: the last step of a chain); at most one of the two.  base: the sample the update starts from (KDPM2's
    second stage) or None.  in_div / clip / x0_out / scaled_out as in sigma_step.  out may be `sample`: the library refuses any other
    overlap.  Returns prev_sample."""
    lib = L.load(); _need_cuda(model_output, sample, noise, base, x0_out, scaled_out, out)
    out = _dense_out("sigma_noise_step", sample, (model_output, noise, base, x0_out, scaled_out), out)
    clip_on, clip_range = _clip_pair(clip)
    s_noise, churn_mul = (1.0, 0.0) if churn is None else churn
    d = L.SigmaNoiseStepDesc(n=sample.numel(), model_output=L.ptr(model_output), sample=L.ptr(sample), noise=L.ptr(noise),
                             base=L.ptr(base), x0_out=L.ptr(x0_out), prev_out=L.ptr(out), scaled_out=L.ptr(scaled_out),
                             sigma_in=float(sigma_in), dt=float(dt), churn=int(churn is not None), s_noise=float(s_noise),
                             churn_mul=float(churn_mul), up=int(sigma_up is not None), sigma_up=float(sigma_up or 0.0),
                             in_div=float(in_div), clip=clip_on, clip_range=clip_range)
    L.check(lib.bd_sigma_noise_step(C.byref(d), L.stream()), "bd_sigma_noise_step")
    return out


def scale_input(x, mul, div, out=None):
    """out = (x * mul) / div (bd_scale_input) over a dense float32 GPU tensor; out may be x."""
    lib = L.load(); _need_cuda(x, out)
    out = _dense_out("scale_input", x, (), out)
    L.check(lib.bd_scale_input(L.ptr(x), x.numel(), float(mul), float(div), L.ptr(out), L.stream()), "bd_scale_input")
    return out


def anp_apply(params, pert_w, pert_b, items, total_rows, out=None):
    """effective parameters of the ANP-perturbed network (bd_anp_apply): a copy of the flat parameter buffer with every conv weight row scaled
    by its channel's pert_w and every conv bias mapped to pert_w * b + pert_b.  items: int64 device tensor [n, 5] (include/bd_hip.h)."""
    lib = L.load(); _need_cuda(params, pert_w, pert_b, items)
    if out is None:
        out = torch.empty_like(params)
    L.check(lib.bd_anp_apply(L.ptr(params), params.numel(), L.ptr(pert_w), L.ptr(pert_b), L.ptr(items), items.shape[0], int(total_rows),
                             L.ptr(out), L.stream()), "bd_anp_apply")
    return out


def anp_grad(params, grad_eff, items, total_rows, grad_w, grad_b, pert_w=None, row_norm=None):
    """gradient of the ANP perturbation from the ordinary flat weight gradient (bd_anp_grad); row_norm: per-channel gradient norm of the
    layer's own weights in the perturbed network (for the reference's clip norm), needs pert_w."""
    lib = L.load(); _need_cuda(params, grad_eff, items, grad_w, grad_b, pert_w, row_norm)
    L.check(lib.bd_anp_grad(L.ptr(params), L.ptr(grad_eff), L.ptr(items), items.shape[0], int(total_rows), L.ptr(pert_w), L.ptr(grad_w),
                            L.ptr(grad_b), L.ptr(row_norm), L.stream()), "bd_anp_grad")
    return grad_w, grad_b


def ssim(preds, target, data_range=1.0):
    """Mean SSIM (torchmetrics defaults, see bd_hip.h) of two [N,C,H,W] float32 GPU tensors with identical strides (any
    layout: a permuted NHWC buffer is fine).  Returns a 0-dim device tensor; batches with N*C > 65535 are chunked."""
    lib = L.load(); _need_cuda(preds, target)
    if preds.shape != target.shape or preds.dim() != 4:
        raise ValueError(f"expected two [N,C,H,W] tensors of the same shape, got {tuple(preds.shape)} and {tuple(target.shape)}")
    if preds.dtype != torch.float32 or target.dtype != torch.float32:
        raise TypeError("ssim: float32 tensors required")
    if preds.stride() != target.stride():
        target = target.contiguous(); preds = preds.contiguous()
    N, Cc, H, W = preds.shape
    per = max(1, 65535 // Cc)
    total = torch.zeros((), dtype=torch.float64, device=preds.device)
    for s0 in range(0, N, per):
        pc, tc = preds[s0:s0 + per], target[s0:s0 + per]
        n = pc.shape[0]
        nbytes = lib.bd_ssim_workspace_bytes(n, Cc, H, W)
        ws = workspace(nbytes, preds.device, "ssim")
        out = torch.empty((), device=preds.device)
        sn, sc, sh, sw = pc.stride()
        L.check(lib.bd_ssim(L.ptr(pc), L.ptr(tc), n, Cc, H, W, sn, sc, sh, sw, float(data_range), L.ptr(out), L.ptr(ws), nbytes, L.stream()),
                "bd_ssim")
        if n == N:
            return out
        total += out.double() * n
    return (total / N).float()


def _image_pair(preds, target, who):
    """bd_image_pair_desc of a float32 [N,C,H,W] GPU tensor of any strides and a target of shape [N,C,H,W], [1,C,H,W] or [C,H,W], which is
    handed over through `expand` strides (0 along a broadcast dimension), never materialised"""
    _need_cuda(preds, target)
    if preds.dim() != 4 or preds.dtype != torch.float32 or preds.numel() == 0:
        raise TypeError(f"{who}: preds must be a non-empty float32 [N,C,H,W] tensor, got {preds.dtype} {tuple(preds.shape)}")
    if target.dtype != torch.float32:
        raise TypeError(f"{who}: target must be float32, got {target.dtype}")
    N, Cc, H, W = preds.shape
    if tuple(target.shape) not in ((N, Cc, H, W), (1, Cc, H, W), (Cc, H, W)):
        raise ValueError(f"{who}: target {tuple(target.shape)} must be [N,C,H,W], [1,C,H,W] or [C,H,W] for preds {tuple(preds.shape)}")
    target = target.expand(N, Cc, H, W)
    d = L.ImagePairDesc(N=N, C=Cc, H=H, W=W, preds=preds.data_ptr(), target=target.data_ptr())
    for i in range(4):
        d.p_stride[i], d.t_stride[i] = preds.stride(i), target.stride(i)
    return d, (preds, target)


def image_loss(preds, target, loss_type="l2"):
    """Per-image mean loss (bd_image_loss): out[n] = mean over (c, h, w) of the element loss of loss_fwd_bwd at preds[n] - target[n].
    preds: float32 [N,C,H,W] GPU tensor of any strides; target: [N,C,H,W], [1,C,H,W] or [C,H,W], broadcast by stride.  Returns a float32
    [N] device tensor whose entries do not depend on the storage order, the batch around an image or the broadcast (bd_hip.h)."""
    lib = L.load()
    if loss_type not in LOSS_TYPES:
        raise NotImplementedError()
    d, _keep = _image_pair(preds, target, "image_loss")
    out = torch.empty(d.N, device=preds.device)
    nbytes = lib.bd_image_loss_workspace_bytes(d.N, d.C, d.H, d.W)
    ws = workspace(nbytes, preds.device, "image_scores") if nbytes else None
    L.check(lib.bd_image_loss(C.byref(d), LOSS_TYPES[loss_type], L.ptr(out), L.ptr(ws), nbytes, L.stream()), "bd_image_loss")
    return out


def ssim_images(preds, target, data_range=1.0):
    """Per-image SSIM (bd_ssim_images, the window and constants of `ssim`): out[n] = mean over the channels and the cropped map of image
    n.  Arguments and independence properties as in image_loss; H, W > 10; any N.  Returns a float32 [N] device tensor."""
    lib = L.load()
    d, _keep = _image_pair(preds, target, "ssim_images")
    out = torch.empty(d.N, device=preds.device)
    nbytes = lib.bd_ssim_images_workspace_bytes(d.N, d.C, d.H, d.W)
    ws = workspace(nbytes, preds.device, "image_scores")
    L.check(lib.bd_ssim_images(C.byref(d), float(data_range), L.ptr(out), L.ptr(ws), nbytes, L.stream()), "bd_ssim_images")
    return out


def vb_terms(x0, x_t, eps, t, tables, clip_denoised=True, want_x0_mse=False):
    """Per-row terms of the variational bound in bits per dimension (bd_vb_terms; the formulas are in bd_hip.h and likelihood.py).
    x0, x_t, eps: float32 [N,C,H,W] GPU tensors of any non-negative strides (x_t and eps may be None when every row is a prior row);
    t: int64 [N] with values in [0, T], row n's own timestep (T = the prior term) -- a HOST tensor is uploaded, a device tensor is copied
    back (a synchronisation), because the launcher checks the values on the host; tables: likelihood.vb_tables(...).
    Returns bits, a float32 [N] device tensor whose entries do not depend on the storage order, the batch around a row or the other
    rows' t; with want_x0_mse (bits, x0_mse), x0_mse[n] the row's mean (x0 - x0_hat)^2."""
    return _vb_terms("vb_terms", x0, x_t, eps, None, t, tables, clip_denoised, want_x0_mse)


def vb_terms_shift(x0, x_t, eps, r, t, tables, clip_denoised=True, want_x0_mse=False):
    """vb_terms along the backdoored chain (bd_vb_terms_shift; bd_hip.h, likelihood.py "The backdoored chain"): a KL row's element is
    (x0 + g_t r - x0_hat)^2, a prior row's (x0 - r)^2, a t = 0 row is vb_terms's and does not read r.
    r: the shift image(s), a float32 GPU tensor [N,C,H,W] of any non-negative strides, or [C,H,W] / [1,C,H,W], one image every row reads
    (by stride 0: nothing is copied); tables: likelihood.vb_tables(..., shift=True, device=...).  Everything else, the returned tensors
    and their independence properties as in vb_terms; x0_mse[n] is the row's mean of the squared term above."""
    return _vb_terms("vb_terms_shift", x0, x_t, eps, r, t, tables, clip_denoised, want_x0_mse)


def _vb_terms(who, x0, x_t, eps, r, t, tables, clip_denoised, want_x0_mse):
    """the checks and the call of vb_terms (r is None) and vb_terms_shift"""
    shift = who == "vb_terms_shift"
    lib = L.load(); _need_cuda(x0, x_t, eps, r)
    if x0.dim() != 4 or x0.dtype != torch.float32 or x0.numel() == 0:
        raise TypeError(f"{who}: x0 must be a non-empty float32 [N,C,H,W] tensor, got {x0.dtype} {tuple(x0.shape)}")
    for name, v in (("x_t", x_t), ("eps", eps)):
        if v is not None and (v.dtype != torch.float32 or v.shape != x0.shape):
            raise TypeError(f"{who}: {name} must be float32 {tuple(x0.shape)}, got {v.dtype} {tuple(v.shape)}")
    N, Cc, H, W = x0.shape
    if shift:
        if not torch.is_tensor(r) or r.dtype != torch.float32 or tuple(r.shape) not in ((N, Cc, H, W), (1, Cc, H, W), (Cc, H, W)):
            raise TypeError(f"{who}: r must be float32 {tuple(x0.shape)}, or one image {(Cc, H, W)} / {(1, Cc, H, W)}, got "
                            f"{getattr(r, 'dtype', type(r))} {tuple(getattr(r, 'shape', ()))}")
        r_stride = (0,) + tuple(r.stride()) if r.dim() == 3 else (r.stride(0) if r.shape[0] == N else 0,) + tuple(r.stride()[1:])
    if not torch.is_tensor(t) or t.dtype != torch.int64 or tuple(t.shape) != (N,):
        raise TypeError(f"{who}: t must be an int64 [{N}] tensor")
    dev = x0.device
    t_host = t.cpu().contiguous()
    t_dev = t.to(dev).contiguous()
    add, mul, ac = tables["add"], tables["mul"], tables["alphas_cumprod"]
    _need_cuda(add, mul, ac)
    T = int(tables["T"])
    if add.numel() != T + 1 or mul.numel() != T + 1 or ac.numel() != T or add.dtype != torch.float32 or mul.dtype != torch.float32 \
            or ac.dtype != torch.float32:
        raise ValueError(f"{who}: tables must hold float32 add / mul of length T + 1 = {T + 1} and alphas_cumprod of length {T}")
    if shift:
        g = tables.get("shift")
        if not torch.is_tensor(g) or g.dtype != torch.float32 or g.numel() != T + 1:
            raise ValueError(f"{who}: tables must hold a float32 shift of length T + 1 = {T + 1} (likelihood.vb_tables(..., shift=True, device=...))")
        _need_cuda(g)
    bits = torch.empty(N, device=dev)
    mse = torch.empty(N, device=dev) if want_x0_mse else None
    common = dict(N=N, C=Cc, H=H, W=W, x0=L.ptr(x0), x_t=L.ptr(x_t), eps=L.ptr(eps), t=L.ptr(t_dev), t_host=t_host.data_ptr(),
                  alphas_cumprod=L.ptr(ac), T=T, term_add=L.ptr(add), term_mul=L.ptr(mul), inv_sigma_dec=float(tables["inv_sigma_dec"]),
                  clip_denoised=int(bool(clip_denoised)), bits=L.ptr(bits), x0_mse=L.ptr(mse))
    d = L.VbTermsShiftDesc(r=L.ptr(r), term_shift=L.ptr(g), **common) if shift else L.VbTermsDesc(**common)
    for i in range(4):
        d.x0_stride[i] = x0.stride(i)
        d.xt_stride[i] = 0 if x_t is None else x_t.stride(i)
        d.eps_stride[i] = 0 if eps is None else eps.stride(i)
        if shift:
            d.r_stride[i] = r_stride[i]
    nbytes = lib.bd_vb_terms_workspace_bytes(N, Cc, H, W)
    ws = workspace(nbytes, dev, "image_scores") if nbytes else None
    entry = "bd_" + who
    L.check(getattr(lib, entry)(C.byref(d), L.ptr(ws), nbytes, L.stream()), entry)
    return (bits, mse) if want_x0_mse else bits


def pairwise_sqdist(x, out=None):
    """d2[i][j] = sum_k (x[i][k] - x[j][k])^2 of the rows of a float32 [N, D] GPU tensor whose last dim is contiguous (any row
    stride): bd_pairwise_sqdist, difference first, square after.  `out`: a float32 [N, >= N] view to write into (last dim
    contiguous); otherwise a new [N, N] tensor.  Returns out[:, :N]."""
    lib = L.load(); _need_cuda(x, out)
    if x.dim() != 2 or x.dtype != torch.float32:
        raise TypeError(f"pairwise_sqdist: a float32 [N, D] tensor is required, got {x.dtype} {tuple(x.shape)}")
    N, D = x.shape
    if out is None:
        out = torch.empty(N, N, device=x.device)
    if out.dim() != 2 or out.dtype != torch.float32 or out.shape[0] != N or out.shape[1] < N:
        raise TypeError(f"pairwise_sqdist: out must be float32 [{N}, >= {N}], got {out.dtype} {tuple(out.shape)}")
    nbytes = lib.bd_pairwise_sqdist_workspace_bytes(N, D)
    ws = workspace(nbytes, x.device, "pairwise") if nbytes else None
    L.check(lib.bd_pairwise_sqdist(L.ptr(x), _ld(x), N, D, L.ptr(out), _ld(out), L.ptr(ws), nbytes, L.stream()), "bd_pairwise_sqdist")
    return out[:, :N]


def _rows2(who, *ts):
    """the checks the bd_cross_* wrappers share: float32 [N, D] GPU tensors with a contiguous last dim and one D"""
    _need_cuda(*ts)
    for t in ts:
        if t.dim() != 2 or t.dtype != torch.float32 or t.shape[0] < 1 or t.shape[1] < 1 or (t.shape[1] > 1 and t.stride(1) != 1):
            raise TypeError(f"{who}: float32 [N, D] tensors with a contiguous last dim are required, got {t.dtype} {tuple(t.shape)}")
    if len({t.shape[1] for t in ts}) != 1:
        raise ValueError(f"{who}: the feature dimensions differ: {[tuple(t.shape) for t in ts]}")


def cross_plan(Na, Nb, D):
    """bd_cross_plan: how the strip kernels cut an (Na, Nb, D) problem, as a dict (strips, col_tiles, csplit, tiles_per_split, csplit_cap)"""
    info = L.CrossPlanInfo()
    L.check(L.load().bd_cross_plan(int(Na), int(Nb), int(D), C.byref(info)), "bd_cross_plan")
    return {f: getattr(info, f) for f, _ in L.CrossPlanInfo._fields_}


def knn_sqradius(x, k):
    """out[i] = the k-th smallest squared distance from row i of a float32 [N, D] GPU tensor to the OTHER rows (self left out by index,
    a duplicate gives 0): bd_knn_sqradius, 1 <= k <= min(16, N - 1).  Returns a float32 [N] tensor."""
    lib = L.load(); _rows2("knn_sqradius", x)
    N, D = x.shape
    out = torch.empty(N, device=x.device)
    nbytes = lib.bd_knn_sqradius_workspace_bytes(N, D, int(k))
    ws = workspace(nbytes, x.device, "cross") if nbytes else None
    L.check(lib.bd_knn_sqradius(L.ptr(x), _ld(x), N, D, int(k), L.ptr(out), L.ptr(ws), nbytes, L.stream()), "bd_knn_sqradius")
    return out


def cross_ksmallest(a, b, k, self_col0=None):
    """out[i] = the k smallest squared distances, ascending, from row i of a to the rows of b (float32 [Na, D] / [Nb, D] GPU tensors),
    column i + self_col0 left out (None: no column is; 0 with a is b: the neighbour lists behind knn_sqradius); +inf where b has
    fewer than k eligible rows: bd_cross_ksmallest, 1 <= k <= 16.  Returns float32 [Na, k]."""
    lib = L.load(); _rows2("cross_ksmallest", a, b)
    (Na, D), Nb = a.shape, b.shape[0]
    out = torch.empty(Na, int(k), device=a.device)
    nbytes = lib.bd_cross_ksmallest_workspace_bytes(Na, Nb, D, int(k))
    ws = workspace(nbytes, a.device, "cross") if nbytes else None
    L.check(lib.bd_cross_ksmallest(L.ptr(a), _ld(a), Na, L.ptr(b), _ld(b), Nb, D, int(k), -Na if self_col0 is None else int(self_col0),
                                   L.ptr(out), L.ptr(ws), nbytes, L.stream()), "bd_cross_ksmallest")
    return out


def cross_count_min(a, b, radius2=None):
    """(count, min_d2) per row of a: count[i] = #{j : d2(a_i, b_j) <= radius2[j]} (int32 [Na]; None without radius2, a float32 [Nb] GPU
    tensor) and min_d2[i] = min_j d2(a_i, b_j) (float32 [Na]): bd_cross_count_min.  No pair is left out."""
    lib = L.load(); _rows2("cross_count_min", a, b); _need_cuda(radius2)
    (Na, D), Nb = a.shape, b.shape[0]
    if radius2 is not None:
        if radius2.dtype != torch.float32 or tuple(radius2.shape) != (Nb,):
            raise TypeError(f"cross_count_min: radius2 must be float32 [{Nb}], got {radius2.dtype} {tuple(radius2.shape)}")
        radius2 = radius2.contiguous()
    count = torch.empty(Na, dtype=torch.int32, device=a.device) if radius2 is not None else None
    min_d2 = torch.empty(Na, device=a.device)
    nbytes = lib.bd_cross_count_min_workspace_bytes(Na, Nb, D)
    ws = workspace(nbytes, a.device, "cross") if nbytes else None
    L.check(lib.bd_cross_count_min(L.ptr(a), _ld(a), Na, L.ptr(b), _ld(b), Nb, D, L.ptr(radius2), L.ptr(count), L.ptr(min_d2), L.ptr(ws),
                                   nbytes, L.stream()), "bd_cross_count_min")
    return count, min_d2


def poly3_rowsum(a, b, exclude_diag=False):
    """rowsum[i] = sum_j (dot(a_i, b_j) / D + 1)^3, the dot product in fp32, the kernel value and the sum in fp64; exclude_diag drops
    j == i (a and b the same set): bd_poly3_rowsum.  Returns a float64 [Na] tensor."""
    lib = L.load(); _rows2("poly3_rowsum", a, b)
    (Na, D), Nb = a.shape, b.shape[0]
    out = torch.empty(Na, dtype=torch.float64, device=a.device)
    nbytes = lib.bd_poly3_rowsum_workspace_bytes(Na, Nb, D)
    ws = workspace(nbytes, a.device, "cross") if nbytes else None
    L.check(lib.bd_poly3_rowsum(L.ptr(a), _ld(a), Na, L.ptr(b), _ld(b), Nb, D, int(bool(exclude_diag)), L.ptr(out), L.ptr(ws), nbytes,
                                L.stream()), "bd_poly3_rowsum")
    return out


def total_variation(images):
    """tv[n] = sum of |vertical| + |horizontal| neighbour differences over all channels of a float32 [N,C,H,W] GPU tensor with any
    strides (NCHW, channels_last, a permuted NHWC buffer): bd_total_variation.  Returns a float32 [N] device tensor."""
    lib = L.load(); _need_cuda(images)
    if images.dim() != 4 or images.dtype != torch.float32:
        raise TypeError(f"total_variation: a float32 [N,C,H,W] tensor is required, got {images.dtype} {tuple(images.shape)}")
    N, Cc, H, W = images.shape
    tv = torch.empty(N, device=images.device)
    sn, sc, sh, sw = images.stride()
    L.check(lib.bd_total_variation(L.ptr(images), N, Cc, H, W, sn, sc, sh, sw, L.ptr(tv), L.stream()), "bd_total_variation")
    return tv


def sumsq(g, out=None):
    lib = L.load(); _need_cuda(g)
    if out is None:
        out = torch.empty((), dtype=torch.float64, device=g.device)
    ws = workspace(lib.bd_reduce_workspace_bytes(), g.device, "reduce")
    L.check(lib.bd_sumsq(L.ptr(g), g.numel(), L.ptr(out), L.ptr(ws), L.stream()), "bd_sumsq")
    return out


def adam_clip(p, g, m, v, sumsq_t, step, lr, max_norm=1.0, betas=(0.9, 0.999), eps=1e-8, grad_norm_out=None, ema=None, one_minus_decay=None):
    """clip + Adam on flat buffers; with `ema` (a flat fp32 shadow of p) and `one_minus_decay`, the EMA update of the shadow rides in the same launch"""
    lib = L.load(); _need_cuda(p, g, m, v, sumsq_t)
    if ema is None:
        if one_minus_decay is not None:
            raise ValueError("adam_clip: one_minus_decay without ema")
        L.check(lib.bd_adam_clip(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), p.numel(), L.ptr(sumsq_t), float(max_norm), float(lr),
                                 float(betas[0]), float(betas[1]), float(eps), int(step), L.ptr(grad_norm_out), L.stream()),
                "bd_adam_clip")
        return
    if one_minus_decay is None:
        raise ValueError("adam_clip: ema needs one_minus_decay")
    _need_cuda(ema)
    _need_flat_f32("adam_clip", ema, p)
    L.check(lib.bd_adam_clip_ema(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(ema), p.numel(), L.ptr(sumsq_t), float(max_norm), float(lr),
                                 float(betas[0]), float(betas[1]), float(eps), int(step), float(one_minus_decay), L.ptr(grad_norm_out),
                                 L.stream()), "bd_adam_clip_ema")


def _need_flat_f32(what, ema, p):
    if ema.dtype != torch.float32 or p.dtype != torch.float32 or not ema.is_contiguous() or not p.is_contiguous() or ema.numel() != p.numel():
        raise TypeError(f"{what}: ema and p must be contiguous float32 tensors of one size, got {ema.dtype} {tuple(ema.shape)} / "
                        f"{p.dtype} {tuple(p.shape)}")


def ema_update(ema, p, one_minus_decay):
    """ema <- ema - fl(omd * fl(ema - p)) in place (EMAModel.step, diffusers/training_utils.py:200-202): three fp32 roundings, one launch"""
    lib = L.load(); _need_cuda(ema, p)
    _need_flat_f32("ema_update", ema, p)
    L.check(lib.bd_ema_update(L.ptr(ema), L.ptr(p), p.numel(), float(one_minus_decay), L.stream()), "bd_ema_update")
    return ema


def tune_set(name, value, check=True):
    """bd_tune_set (run-time tuning knobs of the kernels, e.g. "ps_wg3_slots"; 0 restores the default) + what the C call cannot do: every plan re-lays
    out its workspace on its next call, so the workspaces the live models pool by size are dropped here (callers used to reach into
    model._ws_pool).  Not to be called between a training forward and its backward: the C side refuses a re-layout while saved activations are live."""
    from . import unet
    rc = L.load().bd_tune_set(name.encode() if isinstance(name, str) else name, int(value))
    for m in list(unet.live_models()):
        m._ws_pool = {}
    if check:
        L.check(rc, "bd_tune_set")
    return rc
