"""fp64 numpy restatement of the UniPC sampler (Zhao et al., NeurIPS 2023; the diffusers-0.32.2 algebra of
``UniPCMultistepScheduler`` for ``predict_x0=True``, ``final_sigmas_type="zero"``), written the textbook way: x0 first, then the
corrector UniC on the previous step (D1 differences against the previous x0, ``rhos_c`` by a solve), then the predictor UniP
(D1 differences against the new x0, ``rhos_p``).  TEST INFRASTRUCTURE: it shares no code with ``mvd_amd.scheduler``, which folds
both updates into one affine map for its fused kernel.  ``kernel_map`` restates that kernel's formula (``mvd_op_unipc_step``) with
its rounding-error bound; ``denoise_loop`` is the loop of pipeline.py:119-166 over ``oracle.mvd`` with this sampler.
"""
from __future__ import annotations

import numpy as np
import torch

from tests.sampler_ref import alphas_cumprod, timesteps  # noqa: F401  (the schedule and DPM-Solver++'s grid, which UniPC shares)


class UniPC:
    """sigma = sqrt((1 - a) / a), alpha = 1 / sqrt(sigma^2 + 1), sigma_bar = sigma * alpha, lambda = log alpha - log sigma_bar; the
    sigma after the last timestep is 0.  ``disable_corrector``: step indices i after which (at call i + 1) no corrector runs."""

    def __init__(self, acp, ts, order=2, solver_type="bh2", prediction_type="v_prediction", lower_order_final=True,
                 disable_corrector=()):
        self.ts = [int(t) for t in ts]
        self.sig = [float(np.sqrt((1 - acp[t]) / acp[t])) for t in self.ts] + [0.0]
        self.order, self.solver_type, self.pred = order, solver_type, prediction_type
        self.lower_order_final, self.disable = lower_order_final, set(disable_corrector)
        self.i, self.lower, self.this_order = 0, 0, 0
        self.outs = []              # x0 predictions, oldest first (diffusers' model_outputs)
        self.last_sample = None

    @staticmethod
    def _asl(sigma):
        alpha = 1.0 / np.sqrt(sigma ** 2 + 1.0)
        sbar = sigma * alpha
        return alpha, sbar, (np.inf if sigma == 0.0 else np.log(alpha) - np.log(sbar))

    def _R_b(self, rks, hh, order):
        """diffusers' R (rows of powers of rks) and b, and B(h)"""
        h_phi_1 = np.expm1(hh)
        B = hh if self.solver_type == "bh1" else h_phi_1
        h_phi_k, fact, R, b = h_phi_1 / hh - 1.0, 1.0, [], []
        for j in range(1, order + 1):
            R.append(np.power(rks, j - 1))
            b.append(h_phi_k * fact / B)
            fact *= j + 1
            h_phi_k = h_phi_k / hh - 1.0 / fact
        return np.stack(R), np.array(b), B

    def _corrector(self, model_t, last_sample, order):
        """UniC from sigma_{i-1} to sigma_i: m0 is the x0 at sigma_{i-1}, model_t the x0 just computed at sigma_i"""
        i, m0 = self.i, self.outs[-1]
        alpha_t, sbar_t, lam_t = self._asl(self.sig[i])
        _, sbar_s0, lam_s0 = self._asl(self.sig[i - 1])
        h = lam_t - lam_s0
        rks, D1s = [], []
        for k in range(1, order):
            rk = (self._asl(self.sig[i - 1 - k])[2] - lam_s0) / h
            rks.append(rk)
            D1s.append((self.outs[-(k + 1)] - m0) / rk)
        rks.append(1.0)
        R, b, B = self._R_b(np.array(rks), -h, order)
        rhos = np.array([0.5]) if order == 1 else np.linalg.solve(R, b)
        res = sum((rho * d for rho, d in zip(rhos[:-1], D1s)), 0.0)
        x_t_ = sbar_t / sbar_s0 * last_sample - alpha_t * np.expm1(-h) * m0
        return x_t_ - alpha_t * B * (res + rhos[-1] * (model_t - m0))

    def _predictor(self, x, order):
        """UniP from sigma_i to sigma_{i+1}: m0 is the x0 at sigma_i (the newest entry)"""
        i, m0 = self.i, self.outs[-1]
        alpha_t, sbar_t, lam_t = self._asl(self.sig[i + 1])
        _, sbar_s0, lam_s0 = self._asl(self.sig[i])
        h = lam_t - lam_s0
        x_t_ = sbar_t / sbar_s0 * x - alpha_t * np.expm1(-h) * m0
        if order == 1:
            return x_t_
        assert self.sig[i + 1] != 0.0, "order > 1 onto the zero final sigma"
        rks, D1s = [], []
        for k in range(1, order):
            rk = (self._asl(self.sig[i - k])[2] - lam_s0) / h
            rks.append(rk)
            D1s.append((self.outs[-(k + 1)] - m0) / rk)
        rks.append(1.0)
        R, b, B = self._R_b(np.array(rks), -h, order)
        rhos = np.array([0.5]) if order == 2 else np.linalg.solve(R[:-1, :-1], b[:-1])
        return x_t_ - alpha_t * B * sum(rho * d for rho, d in zip(rhos, D1s))

    def step(self, model_out, x):
        i, n = self.i, len(self.ts)
        alpha_s0, sbar_s0, _ = self._asl(self.sig[i])
        x0 = (x - sbar_s0 * model_out) / alpha_s0 if self.pred == "epsilon" else alpha_s0 * x - sbar_s0 * model_out
        if i > 0 and (i - 1) not in self.disable and self.last_sample is not None:
            x = self._corrector(x0, self.last_sample, self.this_order)
        self.outs = (self.outs + [x0])[-self.order:]
        order = min(self.order, n - i) if self.lower_order_final else self.order
        self.this_order = min(order, self.lower + 1)
        self.last_sample = x
        out = self._predictor(x, self.this_order)
        self.lower = min(self.lower + 1, self.order)
        self.i += 1
        return out


def kernel_map(mo, x, xl, h, k, corr, g=None):
    """``mvd_op_unipc_step``'s formula in fp64 on flat fp64 arrays (numpy, or torch on any device), with the sums of absolute terms
    its fp32 error bound is made of.  ``k``: dict of a0 a1 cx c0 c1 c2 ct px p0 p1 p2 (already rounded to fp32 by the caller);
    ``h``: [h0, h1, h2] (None where the coefficients are 0); ``xl`` None without ``corr``; ``g``: the guidance scale for a stacked
    [u | c] ``mo``.  Returns (y, xc, x0, A_y, A_xc, A_x0) where A_* is the sum of |coefficient * term| over the terms of the
    output, every intermediate replaced by its own A: the kernel's rounding error is at most (operations) * 2^-24 * A."""
    z = x * 0.0
    hv = [z if t is None else t for t in h]
    if g is None:
        m, A_m = mo, abs(mo)
    else:
        n = x.shape[0]
        u, c = mo[:n], mo[n:]
        m, A_m = u + g * (c - u), abs(u) + abs(g) * (abs(c) + abs(u))
    x0 = k["a0"] * m + k["a1"] * x
    A_x0 = abs(k["a0"]) * A_m + abs(k["a1"] * x)
    if corr:
        xc = k["cx"] * xl + k["c0"] * hv[0] + k["c1"] * hv[1] + k["c2"] * hv[2] + k["ct"] * x0
        A_xc = abs(k["cx"] * xl) + abs(k["c0"] * hv[0]) + abs(k["c1"] * hv[1]) + abs(k["c2"] * hv[2]) + abs(k["ct"]) * A_x0
    else:
        xc, A_xc = x, abs(x)
    y = k["px"] * xc + k["p0"] * x0 + k["p1"] * hv[0] + k["p2"] * hv[1]
    A_y = abs(k["px"]) * A_xc + abs(k["p0"]) * A_x0 + abs(k["p1"] * hv[0]) + abs(k["p2"] * hv[1])
    return y, xc, x0, A_y, A_xc, A_x0


def denoise_loop(params, cfg, betas, prompt, negative, latents, src_cam, tgt_cam, src_lat, ts, guidance_scale, fourier_projs,
                 order=2, solver_type="bh2", prediction_type="v_prediction", trace=None, **mv_kwargs):
    """pipeline.py:119-166 on ``oracle.mvd`` (fp32 forward) with the UniPC step in fp64 on the grid ``ts``; returns fp32 latents."""
    from oracle import mvd as M
    acp = alphas_cumprod(betas)
    use_cfg = guidance_scale > 1.0 and negative is not None
    embeds = torch.cat([negative, prompt]) if use_cfg else prompt
    solver = UniPC(acp, ts, order, solver_type, prediction_type)
    x = latents.double().numpy()
    for i, t in enumerate([int(v) for v in ts]):
        x_in = torch.from_numpy(x).float()
        x_in = torch.cat([x_in] * 2) if guidance_scale > 1.0 else x_in
        out = M.multiview_unet_forward(params, cfg, x_in, torch.tensor(t), embeds, src_cam, tgt_cam, src_lat,
                                       fourier_proj=None if fourier_projs is None else fourier_projs[i], **mv_kwargs)
        out = out.double().numpy()
        if guidance_scale > 1.0:
            u, c = np.split(out, 2)
            out = u + guidance_scale * (c - u)
        x = solver.step(out, x)
        if trace is not None:
            trace.append(torch.from_numpy(x).float())
    return torch.from_numpy(x).float()
