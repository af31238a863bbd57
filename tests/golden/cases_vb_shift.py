"""Shared cases of the fixtures of the bound along the backdoored chain (tests/golden/vb_shift.npz): imported by make_golden_vb_shift.py (CPU,
where the reference can be imported) and by tests/test_vb_shift_host.py / tests/test_vb_shift.py.  The schedule, the shapes, the seeds'
base, x0_hat and the decoder element are cases_vb's.

`kernel_formula` restates bd_vb_terms_shift (include/bd_hip.h, baddiffusion_amd/likelihood.py) with torch ops, generic in dtype, the way
cases_vb.kernel_formula restates bd_vb_terms: float64 is the contract (x0_hat formed in float32 from the float32 alphas_cumprod table,
everything after it in float64 with the float64 schedule scalars), float32 the same element arithmetic with the scalars rounded to float32
and the mean in float64; the distance of the two is stored beside each expected value as `d32`.  The element terms, in this order:
    1 <= t < T   s = x0 + g[t] * r;   df = s - x0_hat;   e = df * df
    t = 0        the decoder element of bd_vb_terms (r and g are not read)
    t = T        df = x0 - r;   e = df * df
and x0_mse is the row's mean of df * df (of (x0 - x0_hat)^2 at t = 0)."""
import numpy as np
import torch

from tests.golden import cases_vb as CV

T, LN2 = CV.T, CV.LN2
E2E_TRIGGER_SEED, E2E_TARGET_SEED = 4301, 4302


def shift64():
    """g [T + 1] in float64 from the float32 tables, as likelihood.vb_tables(shift=True) forms it: g_0 = 0, g_T = -1 and
    g_t = (rho_{t-1} - ct_t rho_t) / c0_t with rho_t = 1 - sqrt(abar_t), ct_t = sqrt(alpha_t) (1 - abar_{t-1}) / (1 - abar_t)"""
    betas, alphas, ab = (v.double() for v in CV.schedule())
    abp = torch.cat((torch.ones(1, dtype=torch.float64), ab[:-1]))
    rho = 1 - ab.sqrt()
    rhop = torch.cat((torch.zeros(1, dtype=torch.float64), rho[:-1]))
    c0 = abp.sqrt() * betas / (1 - ab)
    ct = alphas.sqrt() * (1 - abp) / (1 - ab)
    g = torch.zeros(T + 1, dtype=torch.float64)
    g[1:T] = ((rhop - ct * rho) / c0)[1:]
    g[T] = -1.0
    return g


def kernel_formula(x0, x_t, eps, r, ts, vt, clip, dtype):
    """(bits [N], x0_mse [N]) as float64 tensors: rows n of float32 [N,C,H,W] inputs at timesteps ts[n] in [0, T]; r [N,C,H,W] or one
    image [C,H,W] for every row"""
    tab, g = CV.tables64(vt), shift64()
    rnd = lambda v: torch.as_tensor(v, dtype=torch.float64).to(dtype).double()       # a schedule scalar as this dtype holds it
    bits, mse = [], []
    for n, t in enumerate(int(t) for t in ts):
        v = x0[n].to(dtype)
        rr = (r if r.dim() == 3 else r[n]).to(dtype)
        if t == T:
            df = v - rr
            e = m2 = df * df
        else:
            xh = CV.x0_hat(x_t[n], eps[n], t, clip)
            if t == 0:
                df = v - xh.to(dtype)
                m2 = df * df
                e = CV.dec_nll(x0[n], xh, float(rnd(tab["inv_sigma_dec"])), dtype)
            else:
                s = v + rnd(g[t]).to(dtype) * rr
                df = s - xh.to(dtype)
                e = m2 = df * df
        bits.append((rnd(tab["add"][t]) + rnd(tab["mul"][t]) * e.double().mean()) / LN2)
        mse.append(m2.double().mean())
    return torch.stack(bits), torch.stack(mse)


def r_coef(t):
    """R_coef_t = (1 - sqrt(alpha_t)) sqrt(1 - abar_t) / (1 - alpha_t) as a 0-dim float32 tensor, the operations of the q_sample kernels
    (numpy's correctly rounded scalar sqrt, see cases_vb.coef)"""
    al = np.float32(CV.schedule()[1][t].item())
    ab = np.float32(CV.schedule()[2][t].item())
    one = np.float32(1.0)
    return torch.tensor((one - np.sqrt(al)) * np.sqrt(one - ab) / (one - al))


def make_rows(seed, N, shape, ts, s=0.1, s0=0.01):
    """float32 (x0, x_t, eps, r) [N, *shape]: x0 and r data-like from random uint8, x_t the shifted chain's sample
    sqrt(abar_t) x0 + sqrt(1 - abar_t) noise + (1 - sqrt(abar_t)) r, and eps = noise + R_coef_t r - (sqrt(abar_t) / sqrt(1 - abar_t)) scale err:
    the training target of the backdoored chain plus an error, so that the unclamped prediction is x0 + g_t r + scale err (scale = s0 in
    t = 0 rows, s elsewhere) -- the regime in which the KL element is a small difference of large numbers at large t.  Prior rows keep noise
    / err in x_t / eps: the kernel must not read them.  Integer draws and correctly rounded float32 operations only."""
    g = torch.Generator().manual_seed(seed)
    full = (N,) + tuple(shape)
    x0 = CV.data_x0(torch.randint(0, 256, full, generator=g))
    r = CV.data_x0(torch.randint(0, 256, full, generator=g))
    noise, err = CV.exact_randn(full, g), CV.exact_randn(full, g)
    x_t, eps = noise.clone(), err.clone()
    for n, t in enumerate(int(t) for t in ts):
        if t < T:
            sa, sb = CV.coef(t)
            x_t[n] = (sa * x0[n] + sb * noise[n]) + (1.0 - sa) * r[n]
            eps[n] = (r_coef(t) * r[n] + noise[n]) - (sa / sb) * (s0 if t == 0 else s) * err[n]
    return x0, x_t, eps, r


def kernel_cases():
    """(tag, shape, N, ts, variance_type, clip, seed): cases_vb's shape cases on seeds of their own"""
    for tag, shape, N, ts, vt, clip, seed in CV.kernel_cases():
        yield tag, shape, N, ts, vt, clip, 5000 + seed


# ---------------------------------------------------------------------------------------------------- end to end
def e2e_backdoor(C=3, S=16):
    """(trigger, target) float32 [C, S, S] in [-1, 1]: a 4 x 4 box of random grey levels in the lower right corner on the -1 background
    (the mask of ops.poison_qsample is trigger > -1), and a data-like target image"""
    trigger = torch.full((C, S, S), -1.0)
    u = torch.randint(1, 256, (C, 4, 4), generator=torch.Generator().manual_seed(E2E_TRIGGER_SEED))
    trigger[:, S - 6: S - 2, S - 6: S - 2] = CV.data_x0(u)
    target = CV.data_x0(torch.randint(0, 256, (C, S, S), generator=torch.Generator().manual_seed(E2E_TARGET_SEED)))
    return trigger, target


def e2e_rows():
    """(x0, r) float32 [E2E_N, C, S, S] of the poisoned end-to-end rows: x0 the target, r = m x + (1 - m) g of the carriers
    cases_vb.e2e_clean() (m = 0 where the trigger is above -1), the blend of the reference's dataset transform"""
    trigger, target = e2e_backdoor()
    x = CV.data_x0(CV.e2e_clean()).permute(0, 3, 1, 2).contiguous()
    m = torch.where(trigger > -1.0, torch.zeros_like(trigger), torch.ones_like(trigger))
    r = m * x + (1.0 - m) * trigger
    return target[None].repeat(CV.E2E_N, 1, 1, 1).contiguous(), r
