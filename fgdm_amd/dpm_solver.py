"""Host-side mirror of ldm/models/diffusion/dpm_solver/dpm_solver.py: NoiseScheduleVP, model_wrapper, DPM_Solver, with the
reference's signatures.

  NoiseScheduleVP   <- dpm_solver.py:6-175   (the discrete schedule; float32 scalars on the host)
  model_wrapper     <- dpm_solver.py:177-348 (model_type 'noise'; guidance 'uncond' / 'classifier-free')
  DPM_Solver        <- dpm_solver.py:351-1124 (multistep and singlestep solvers of order 1..3, both predictions, the three step
                       spacings, both solver types, t_start / t_end, lower_order_final, denoise_to_zero)

Every update of the family is a linear combination of x and of model values kept from earlier evaluations, so a whole sampling
compiles into a flat PROGRAM with one record per network evaluation (dpm_solver_program).  Both routes read that program and nothing
else: the per-step route below (any callable model_fn; one launch of k_dpm_program_step per record through engine.dpm_program_step)
and the device loop (DPM_Solver(..., device_loop=True) -> Engine.sample_dpm_solver / fgdm_sample_dpm_solver: the whole sampling in
one engine call, when model_fn is the object model_wrapper returns and samplers._loop_plan takes its conditionings).
Not carried over, and refused by name: the continuous schedules, classifier guidance, the 'x_start' / 'v' / 'score' model types,
dynamic thresholding, method='adaptive' (a data-dependent step control: it needs the host between evaluations).
"""
import numpy as np
import torch

from . import engine as _k
from .samplers import _DiscreteVPSchedule, _loop_plan

# the planes a term of a record's update can name (FGDM_DPM_PLANE_* of include/fgdm.h)
PLANE_BASE, PLANE_HIST0, PLANE_HIST1, PLANE_HIST2, PLANE_M = 0, 1, 2, 3, 4
# where the update's result goes (FGDM_DPM_DEST_*)
DEST_STATE, DEST_EVAL = 1, 2
MAX_TERMS = 5

_f32 = np.float32


class NoiseScheduleVP(_DiscreteVPSchedule):
    """dpm_solver.py:6-175 for schedule='discrete': marginal_log_mean_coeff / marginal_alpha / marginal_std / marginal_lambda of
    _DiscreteVPSchedule plus inverse_lambda; scalars in, numpy float32 scalars out."""

    def __init__(self, schedule='discrete', betas=None, alphas_cumprod=None, continuous_beta_0=0.1, continuous_beta_1=20.):
        if schedule in ('linear', 'cosine'):
            raise NotImplementedError(f"NoiseScheduleVP(schedule='{schedule}'): the continuous-time schedules are not carried over; "
                                      "only schedule='discrete' is")
        if schedule != 'discrete':
            raise ValueError("Unsupported noise schedule {}. The schedule needs to be 'discrete' or 'linear' or 'cosine'".format(schedule))
        self.schedule = schedule
        host = lambda v: v.detach().float().cpu().numpy() if torch.is_tensor(v) else np.asarray(v, dtype=np.float32)
        if betas is not None:                                                    # dpm_solver.py:100-101
            ac = np.exp(np.cumsum(np.log(_f32(1.) - host(betas)), dtype=np.float32))
        else:
            assert alphas_cumprod is not None
            ac = host(alphas_cumprod)
        super().__init__(ac)

    @staticmethod
    def _interp(x, xp, yp):
        """interpolate_fn (dpm_solver.py:1132-1171) for one scalar over ascending keypoints, as marginal_log_mean_coeff does it"""
        K = len(xp)
        idx = int(np.searchsorted(xp, x, side='left'))
        i0 = 0 if idx == 0 else (K - 2 if idx >= K else idx - 1)
        x0, x1, y0, y1 = xp[i0], xp[i0 + 1], yp[i0], yp[i0 + 1]
        return _f32(y0 + (x - x0) * (y1 - y0) / (x1 - x0))

    def inverse_lambda(self, lamb):
        """t of a half-logSNR lambda (dpm_solver.py:166-169): log alpha = -0.5 logaddexp(0, -2 lambda), then the inverse of the
        piecewise-linear log alpha(t)"""
        log_alpha = _f32(-0.5) * np.logaddexp(_f32(0.), _f32(-2.) * _f32(lamb), dtype=np.float32)
        return self._interp(_f32(log_alpha), self.log_alpha[::-1], self.t_array[::-1])


class _WrappedModel:
    """What model_wrapper returns: the noise prediction model over continuous time (dpm_solver.py:321-344) as a callable OBJECT that
    still carries the model, both conditions and the scale, so that DPM_Solver can hand a whole sampling to the engine.
    `ldm`: the LatentDiffusion / ControlLDM mirror behind `model` (the model itself, or the owner of a bound apply_model), else None."""

    def __init__(self, model, noise_schedule, model_kwargs, guidance_type, condition, unconditional_condition, guidance_scale):
        self.model, self.noise_schedule, self.model_kwargs = model, noise_schedule, dict(model_kwargs or {})
        self.guidance_type, self.guidance_scale = guidance_type, guidance_scale
        self.condition, self.unconditional_condition = condition, unconditional_condition
        owner = model if hasattr(model, 'apply_model') else getattr(model, '__self__', None)
        self.ldm = owner if hasattr(owner, 'apply_model') and getattr(model, '__name__', 'apply_model') == 'apply_model' else None
        self._call = model.apply_model if hasattr(model, 'apply_model') else model
        self._c_in = None

    @property
    def cfg_on(self):
        return self.guidance_type == 'classifier-free' and self.guidance_scale != 1. and self.unconditional_condition is not None

    def _joined(self):
        """cat([unconditional_condition, condition]) (dpm_solver.py:342), the SAME tensor object in every evaluation"""
        uc, c = self.unconditional_condition, self.condition
        key = (id(uc), uc._version, id(c), c._version)
        if self._c_in is None or self._c_in[0] != key:
            self._c_in = (key, torch.cat([uc, c]))
        return self._c_in[1]

    def eval_pair(self, x, t_input):
        """(e_cond, e_uncond or None) at the model's time input t_input [B]: one 2B batch under guidance (dpm_solver.py:340-343)"""
        kw = self.model_kwargs
        if self.guidance_type == 'uncond':
            return self._call(x, t_input, **kw), None
        if not self.cfg_on:
            return self._call(x, t_input, self.condition, **kw), None
        if getattr(self.ldm, 'engine', None) is not None:
            kw = dict(kw, cfg_pairs=True)       # rows b and b + B differ only in the context (samplers._eval_pair)
        e_u, e_c = self._call(torch.cat([x] * 2), torch.cat([t_input] * 2), self._joined(), **kw).chunk(2)
        return e_c.contiguous(), e_u.contiguous()

    def __call__(self, x, t_continuous):
        if t_continuous.reshape((-1,)).shape[0] == 1:
            t_continuous = t_continuous.expand((x.shape[0]))
        t_input = (t_continuous - 1. / self.noise_schedule.total_N) * 1000.      # get_model_input_time, dpm_solver.py:278-287
        e_c, e_u = self.eval_pair(x, t_input)
        return e_c if e_u is None else _k.cfg_combine(e_c, e_u, self.guidance_scale)


def model_wrapper(model, noise_schedule, model_type="noise", model_kwargs={}, guidance_type="uncond", condition=None,
                  unconditional_condition=None, guidance_scale=1., classifier_fn=None, classifier_kwargs={}):
    """dpm_solver.py:177-348.  model: a callable (x, t_input[, cond], **model_kwargs) -> eps, or a LatentDiffusion / ControlLDM
    mirror (its apply_model is called); handing over the mirror or its bound apply_model is what lets DPM_Solver(device_loop=True)
    find the engine."""
    assert model_type in ["noise", "x_start", "v", "score"]
    assert guidance_type in ["uncond", "classifier", "classifier-free"]
    if model_type != "noise":
        raise NotImplementedError(f"model_wrapper(model_type='{model_type}'): only noise-prediction models (model_type='noise') are carried over")
    if guidance_type == "classifier":
        raise NotImplementedError("model_wrapper(guidance_type='classifier'): classifier guidance needs the classifier's gradient "
                                  "(autograd) in every evaluation; 'uncond' and 'classifier-free' are carried over")
    return _WrappedModel(model, noise_schedule, model_kwargs, guidance_type, condition, unconditional_condition, guidance_scale)


# ---------------------------------------------------------------------------------------------------- the program
def get_time_steps(ns, skip_type, t_T, t_0, N):
    """DPM_Solver.get_time_steps (dpm_solver.py:410-437): N + 1 float32 times from t_T to t_0"""
    if skip_type == 'logSNR':
        lam = np.linspace(ns.marginal_lambda(t_T), ns.marginal_lambda(t_0), N + 1, dtype=np.float32)
        return np.asarray([ns.inverse_lambda(v) for v in lam], dtype=np.float32)
    if skip_type == 'time_uniform':
        return np.linspace(t_T, t_0, N + 1, dtype=np.float32)
    if skip_type == 'time_quadratic':
        return np.linspace(t_T ** 0.5, t_0 ** 0.5, N + 1, dtype=np.float32) ** 2
    raise ValueError("Unsupported skip_type {}, need to be 'logSNR' or 'time_uniform' or 'time_quadratic'".format(skip_type))


def singlestep_orders(steps, order):
    """the orders of get_orders_and_timesteps_for_singlestep_solver (dpm_solver.py:471-490)"""
    if order == 3:
        K = steps // 3 + 1
        return [3] * (K - 2) + [2, 1] if steps % 3 == 0 else [3] * (K - 1) + ([1] if steps % 3 == 1 else [2])
    if order == 2:
        return [2] * (steps // 2) if steps % 2 == 0 else [2] * (steps // 2) + [1]
    if order == 1:
        return [1] * steps
    raise ValueError("'order' must be '1' or '2' or '3'.")


class _Builder:
    """the coefficient algebra of the updates (dpm_solver.py:504-857), every scalar a numpy float32 as the reference's float32
    tensors; an update is (coefficient of x, [(model index, coefficient), ...])"""

    def __init__(self, ns, predict_x0, solver_type):
        self.ns, self.px0, self.taylor = ns, bool(predict_x0), solver_type == 'taylor'

    def _base(self, s, t, expm1_form):
        """(h, coefficient of x, c2 with x_t = cx x - c2 model_s + ...) of a step from s to t.  The first-order and the singlestep
        updates write phi_1 as expm1(.), the multistep ones as exp(.) - 1, like the reference"""
        ns = self.ns
        h = ns.marginal_lambda(t) - ns.marginal_lambda(s)
        if self.px0:
            phi_1 = _f32(np.expm1(-h)) if expm1_form else _f32(np.exp(-h)) - _f32(1.)
            return h, ns.marginal_std(t) / ns.marginal_std(s), ns.marginal_alpha(t) * phi_1, phi_1
        phi_1 = _f32(np.expm1(h)) if expm1_form else _f32(np.exp(h)) - _f32(1.)
        cx = _f32(np.exp(ns.marginal_log_mean_coeff(t) - ns.marginal_log_mean_coeff(s)))
        return h, cx, ns.marginal_std(t) * phi_1, phi_1

    def _scale(self, t):
        """alpha_t (data prediction) or sigma_t (noise prediction): the factor of every phi term"""
        return self.ns.marginal_alpha(t) if self.px0 else self.ns.marginal_std(t)

    def first(self, s, t):                                                       # dpm_solver.py:504-549
        _, cx, c2, _ = self._base(s, t, True)
        return cx, [(0, -c2)]

    def _phi2_ms(self, h):
        """the multistep forms (exp(-h) - 1) / h + 1 and (exp(h) - 1) / h - 1 (dpm_solver.py:795, 808, 847, 854)"""
        return (_f32(np.exp(-h)) - _f32(1.)) / h + _f32(1.) if self.px0 else (_f32(np.exp(h)) - _f32(1.)) / h - _f32(1.)

    def multistep_second(self, t1, t0, t):                                       # dpm_solver.py:755-810; models: 0 newest, 1 before it
        ns = self.ns
        h, cx, c2, _ = self._base(t0, t, False)
        r0 = (ns.marginal_lambda(t0) - ns.marginal_lambda(t1)) / h
        if not self.taylor:
            d = -(_f32(0.5) * c2)                                                # the signed coefficient of D1_0 = (m0 - m1) / r0
        else:
            d = self._scale(t) * self._phi2_ms(h) * (_f32(1.) if self.px0 else _f32(-1.))
        return cx, [(0, -c2 + d / r0), (1, -(d / r0))]

    def multistep_third(self, t2, t1, t0, t):                                    # dpm_solver.py:812-857; models: 0 newest ... 2 oldest
        ns = self.ns
        h, cx, c2, _ = self._base(t0, t, False)
        l2, l1, l0 = ns.marginal_lambda(t2), ns.marginal_lambda(t1), ns.marginal_lambda(t0)
        r0, r1 = (l0 - l1) / h, (l1 - l2) / h
        if self.px0:
            a = self._scale(t) * self._phi2_ms(h)
            b = -(self._scale(t) * ((_f32(np.exp(-h)) - _f32(1.) + h) / h ** 2 - _f32(0.5)))
        else:
            a = -(self._scale(t) * self._phi2_ms(h))
            b = -(self._scale(t) * ((_f32(np.exp(h)) - _f32(1.) - h) / h ** 2 - _f32(0.5)))
        # D1 = D1_0 + k (D1_0 - D1_1), D2 = q (D1_0 - D1_1);  D1_0 = (m0 - m1) / r0, D1_1 = (m1 - m2) / r1
        k, q = r0 / (r0 + r1), _f32(1.) / (r0 + r1)
        u, v = a * (_f32(1.) + k) + b * q, -(a * k) - b * q
        return cx, [(0, -c2 + u / r0), (1, v / r1 - u / r0), (2, -(v / r1))]

    def _to_inner(self, s, h, r):
        """an intermediate point of a singlestep update: (its time, x_s1 = cx x + cm model_s) (dpm_solver.py:576-591, 611-614)"""
        ns = self.ns
        s1 = ns.inverse_lambda(ns.marginal_lambda(s) + r * h)
        if self.px0:
            return s1, ns.marginal_std(s1) / ns.marginal_std(s), -(ns.marginal_alpha(s1) * _f32(np.expm1(-r * h)))
        cx = _f32(np.exp(ns.marginal_log_mean_coeff(s1) - ns.marginal_log_mean_coeff(s)))
        return s1, cx, -(ns.marginal_std(s1) * _f32(np.expm1(r * h)))

    def singlestep_second(self, s, t, r1):                                       # dpm_solver.py:551-631; models: 0 at s, 1 at s1
        r1 = _f32(0.5) if r1 is None else r1
        h, cx, c2, phi_1 = self._base(s, t, True)
        s1, cx1, cm1 = self._to_inner(s, h, r1)
        if not self.taylor:
            d = -((_f32(0.5) / r1) * c2)                                         # the signed coefficient of (model_s1 - model_s)
        else:
            d = (_f32(1.) / r1) * (self._scale(t) * self._phi2_ms(h)) * (_f32(1.) if self.px0 else _f32(-1.))
        return [(s1, cx1, [(0, cm1)])], (cx, [(0, -c2 - d), (1, d)])

    def singlestep_third(self, s, t, r1, r2):                                    # dpm_solver.py:633-753; models: 0 at s, 1 at s1, 2 at s2
        r1 = _f32(1. / 3.) if r1 is None else r1
        r2 = _f32(2. / 3.) if r2 is None else r2
        ns, sign = self.ns, (_f32(1.) if self.px0 else _f32(-1.))
        h, cx, c2, phi_1 = self._base(s, t, True)
        s1, cx1, cm1 = self._to_inner(s, h, r1)
        s2, cx2, cm2 = self._to_inner(s, h, r2)
        em = _f32(np.expm1(-r2 * h)) if self.px0 else _f32(np.expm1(r2 * h))
        phi_22 = em / (r2 * h) + sign
        phi_2 = phi_1 / h + sign
        phi_3 = phi_2 / h - _f32(0.5)
        e = sign * (r2 / r1 * (self._scale(s2) * phi_22))                        # the signed coefficient of (model_s1 - model_s) in x_s2
        inner = [(s1, cx1, [(0, cm1)]), (s2, cx2, [(0, cm2 - e), (1, e)])]
        if not self.taylor:
            f = sign * ((_f32(1.) / r2) * (self._scale(t) * phi_2))              # ... of (model_s2 - model_s) in x_t
            return inner, (cx, [(0, -c2 - f), (2, f)])
        # D1_0 = (m1 - m0) / r1, D1_1 = (m2 - m0) / r2, D1 = (r2 D1_0 - r1 D1_1) / (r2 - r1), D2 = 2 (D1_1 - D1_0) / (r2 - r1)
        a, b = sign * (self._scale(t) * phi_2), -(self._scale(t) * phi_3)
        u = (a * r2 - _f32(2.) * b) / (r2 - r1)
        v = (_f32(2.) * b - a * r1) / (r2 - r1)
        return inner, (cx, [(0, -c2 - u / r1 - v / r2), (1, u / r1), (2, v / r2)])


def dpm_solver_program(ns, steps=20, order=3, skip_type='time_uniform', method='singlestep', predict_x0=False,
                       lower_order_final=True, denoise_to_zero=False, solver_type='dpm_solver', t_start=None, t_end=None):
    """DPM_Solver.sample (dpm_solver.py:965-1124) compiled into a flat program: a dict of equally long lists, one entry per network
    evaluation k, in float32 arithmetic handed out as Python floats.  Evaluation k runs the network on the current evaluation
    input x_eval at the time input t_float[k]; then ONE pass over the elements (k_dpm_program_step) does
      m   = eps                                  (conv_x[k] == 0: the noise prediction), or
            conv_x[k] x_eval + conv_e[k] eps     (the data prediction (x - sigma eps) / alpha, dpm_solver.py:386-399)
      m  -> history plane slot[k] (0..2; -1: no later record reads it, nothing is stored)
      acc = sum_j coef[k][j] p_j over the nterms[k] (1..5) terms, p_j the plane plane[k][j]: PLANE_BASE (the state x), PLANE_HIST0..2
            (a model value kept by an earlier record) or PLANE_M (the m of this record); term 0 is rounded on its own, every further
            term is fused into the sum in order.  The newest model value of the update comes first and x second, so that a first-order
            update rounds as the existing samplers' axpby(x, cx, m, cm) does: fma(cx, x, round(cm m))
      acc -> the state x and the next evaluation input (dest[k] == DEST_STATE), or the next evaluation input only (DEST_EVAL: the
            intermediate points s1, s2 of the singlestep solvers, where the x at s must survive).
    't' holds the continuous time of every evaluation (what a bare callable model_fn receives).  The per-step route and the device
    loop (fgdm_sample_dpm_solver) both read this program and nothing else, so they cannot drift apart."""
    if method == 'adaptive':
        raise NotImplementedError("DPM_Solver.sample(method='adaptive'): the adaptive step-size solver decides every step from the data "
                                  "(an error norm of x) and cannot be compiled into a program; 'multistep', 'singlestep' and "
                                  "'singlestep_fixed' are carried over")
    if method not in ('multistep', 'singlestep', 'singlestep_fixed'):
        raise ValueError(f"unknown method '{method}'")
    if solver_type not in ('dpm_solver', 'taylor'):
        raise ValueError("'solver_type' must be either 'dpm_solver' or 'taylor', got {}".format(solver_type))
    if order not in (1, 2, 3):
        raise ValueError("Solver order must be 1 or 2 or 3, got {}".format(order))
    t_0 = 1. / ns.total_N if t_end is None else t_end
    t_T = ns.T if t_start is None else t_start
    b = _Builder(ns, predict_x0, solver_type)
    prog = {k: [] for k in ('t', 't_float', 'conv_x', 'conv_e', 'slot', 'nterms', 'plane', 'coef', 'dest')}

    def emit(t, slot, cx, terms, dest, where):
        """one record: the evaluation at t, its model value to `slot`, then x' = cx x + sum coef * model; terms: [(slot or PLANE_M
        given as -1, coefficient)]; `where`: model index -> history slot, the current evaluation mapped to the register"""
        t = _f32(t)
        prog['t'].append(float(t))
        prog['t_float'].append(float((t - _f32(1. / ns.total_N)) * _f32(1000.)))      # get_model_input_time, dpm_solver.py:278-287
        if predict_x0:
            a, sg = ns.marginal_alpha(t), ns.marginal_std(t)
            prog['conv_x'].append(float(_f32(1.) / a))
            prog['conv_e'].append(float(-sg / a))
        else:
            prog['conv_x'].append(0.0)
            prog['conv_e'].append(1.0)
        # the first model term leads and x follows it: fma(cx, x, round(c m)), the rounding of the existing updates' axpby(x, cx, m, c)
        planes, coefs = [where[terms[0][0]]], [float(terms[0][1])]
        if cx is not None:
            planes.append(PLANE_BASE)
            coefs.append(float(cx))
        for idx, c in terms[1:]:
            planes.append(where[idx])
            coefs.append(float(c))
        n = len(planes)
        assert 1 <= n <= MAX_TERMS
        prog['slot'].append(slot)
        prog['nterms'].append(n)
        prog['plane'].append(planes + [PLANE_BASE] * (MAX_TERMS - n))
        prog['coef'].append(coefs + [0.0] * (MAX_TERMS - n))
        prog['dest'].append(dest)

    if method == 'multistep':
        assert steps >= order
        ts = get_time_steps(ns, skip_type, t_T, t_0, steps)
        for k in range(steps):                                                   # the evaluation at ts[k], then the update to ts[k + 1]
            step = k + 1                                                         # the reference's loop variable of this update
            if step < order:
                step_order = step                                                # init orders 1 .. order - 1 (dpm_solver.py:1086-1090)
            else:
                step_order = min(order, steps + 1 - step) if lower_order_final and steps < 15 else order
            # model index j (0 newest) -> where it lives: the evaluation k - j went to history slot (k - j) % 3
            where = {0: PLANE_M, 1: PLANE_HIST0 + (k - 1) % 3, 2: PLANE_HIST0 + (k - 2) % 3}
            if step_order == 1:
                cx, terms = b.first(ts[k], ts[k + 1])
            elif step_order == 2:
                cx, terms = b.multistep_second(ts[k - 1], ts[k], ts[k + 1])
            else:
                cx, terms = b.multistep_third(ts[k - 2], ts[k - 1], ts[k], ts[k + 1])
            emit(ts[k], k % 3, cx, terms, DEST_STATE, where)
    else:
        if method == 'singlestep':
            orders = singlestep_orders(steps, order)
            if skip_type == 'logSNR':                                            # one logSNR interval per solver step (dpm_solver.py:491-493)
                outer = get_time_steps(ns, skip_type, t_T, t_0, len(orders))
            else:
                outer = get_time_steps(ns, skip_type, t_T, t_0, steps)[np.cumsum([0] + orders)]
        else:
            orders = [order] * (steps // order)
            outer = get_time_steps(ns, skip_type, t_T, t_0, len(orders))
        for i, o in enumerate(orders):
            s, t = outer[i], outer[i + 1]
            inner_t = get_time_steps(ns, skip_type, float(s), float(t), o)
            lam = [ns.marginal_lambda(v) for v in inner_t]
            h = lam[-1] - lam[0]
            r1 = None if o <= 1 else (lam[1] - lam[0]) / h
            r2 = None if o <= 2 else (lam[2] - lam[0]) / h
            if o == 1:
                inner, (cx, terms) = [], b.first(s, t)
            elif o == 2:
                inner, (cx, terms) = b.singlestep_second(s, t, r1)
            else:
                inner, (cx, terms) = b.singlestep_third(s, t, r1, r2)
            # the evaluation j of this step (at s, s1, s2) goes to history slot j; the newest one is still in the register
            points = [s] + [p[0] for p in inner]
            updates = [(p[1], p[2], DEST_EVAL) for p in inner] + [(cx, terms, DEST_STATE)]
            for j, (pt, (ucx, uterms, dest)) in enumerate(zip(points, updates)):
                where = {q: (PLANE_M if q == j else PLANE_HIST0 + q) for q in range(j + 1)}
                emit(pt, j, ucx, uterms, dest, where)
    if denoise_to_zero:                                                          # dpm_solver.py:498-502, 1122-1123: x = data prediction at t_0
        was = predict_x0
        predict_x0 = True
        emit(_f32(t_0), -1, None, [(0, _f32(1.))], DEST_STATE, {0: PLANE_M})
        predict_x0 = was
    # a model value no later record reads is not stored
    K = len(prog['slot'])
    for k in range(K):
        slot, read = prog['slot'][k], False
        if slot < 0:
            continue
        for q in range(k + 1, K):
            if PLANE_HIST0 + slot in prog['plane'][q][:prog['nterms'][q]]:
                read = True
            if read or prog['slot'][q] == slot:
                break
        if not read:
            prog['slot'][k] = -1
    return prog


def program_error(prog):
    """None, or what is wrong with a program (the checks fgdm_sample_dpm_solver makes before its first launch)"""
    written = set()
    for k in range(len(prog['t_float'])):
        n = prog['nterms'][k]
        if not 1 <= n <= MAX_TERMS:
            return f'record {k}: nterms {n} is outside 1..{MAX_TERMS}'
        for p in prog['plane'][k][:n]:
            if not PLANE_BASE <= p <= PLANE_M:
                return f'record {k}: unknown plane {p}'
            if PLANE_HIST0 <= p <= PLANE_HIST2 and p - PLANE_HIST0 not in written:
                return f'record {k}: reads history slot {p - PLANE_HIST0}, which no earlier record wrote'
        if not -1 <= prog['slot'][k] <= 2:
            return f'record {k}: slot {prog["slot"][k]} is outside -1..2'
        if prog['dest'][k] not in (DEST_STATE, DEST_EVAL):
            return f'record {k}: unknown destination {prog["dest"][k]}'
        if prog['slot'][k] >= 0:
            written.add(prog['slot'][k])
    if not prog['t_float']:
        return 'an empty program'
    if prog['dest'][-1] != DEST_STATE:
        return 'the last record does not write the state'
    return None


class DPM_Solver:
    """dpm_solver.py:351-1124.  model_fn: the object model_wrapper returns, or any callable (x, t_continuous) -> eps.
    device_loop=True (an added keyword, off by default): sample() hands the whole sampling to the engine (fgdm_sample_dpm_solver)
    when model_fn is the wrapper's object over a LatentDiffusion / ControlLDM mirror and samplers._loop_plan takes its
    conditionings -- the rule of the other device loops; same program, same bits as the per-step route."""

    def __init__(self, model_fn, noise_schedule, predict_x0=False, thresholding=False, max_val=1., device_loop=False):
        if thresholding:
            raise NotImplementedError('DPM_Solver(thresholding=True): dynamic thresholding (a per-sample quantile of the data prediction, '
                                      'for pixel-space models) is not carried over')
        self.model = model_fn
        self.noise_schedule = noise_schedule
        self.predict_x0 = predict_x0
        self.thresholding = thresholding
        self.max_val = max_val
        self.device_loop = bool(device_loop)

    def _plan(self, x, prog):
        """None (per-step route), or (engine, ctx, uctx, flags, control_scales) of the device loop"""
        w = self.model
        if not self.device_loop or not isinstance(w, _WrappedModel) or w.ldm is None or w.guidance_type != 'classifier-free':
            return None
        plan = _loop_plan(w.ldm, None, w.condition, w.unconditional_condition, [w.guidance_scale] * len(prog['t_float']), None, None, x,
                          False, w.model_kwargs, entry='sample_dpm_solver')
        return None if plan is None else (w.ldm.engine, *plan)

    def sample(self, x, steps=20, t_start=None, t_end=None, order=3, skip_type='time_uniform', method='singlestep',
               lower_order_final=True, denoise_to_zero=False, solver_type='dpm_solver', atol=0.0078, rtol=0.05):
        prog = dpm_solver_program(self.noise_schedule, steps, order, skip_type, method, self.predict_x0, lower_order_final,
                                  denoise_to_zero, solver_type, t_start, t_end)
        plan = self._plan(x, prog)
        if plan is not None:
            engine, ctx, uctx, flags, control_scales = plan
            scale = self.model.guidance_scale if uctx is not None else 1.0
            return engine.sample_dpm_solver(x, ctx, uctx, scale, prog, control_scales=control_scales, flags=flags).to(x.device)
        return run_program(prog, self.model, x)


def run_program(prog, model_fn, x):
    """The per-step route: per record one evaluation of model_fn and one launch of k_dpm_program_step (engine.dpm_program_step)."""
    wrapped = isinstance(model_fn, _WrappedModel)
    x = x.to(torch.float32).contiguous()
    x_eval, hist = x, [None] * 3
    for k in range(len(prog['t_float'])):
        if wrapped:
            t_in = torch.full((x.shape[0],), prog['t_float'][k], device=x.device, dtype=torch.float32)
            e_c, e_u = model_fn.eval_pair(x_eval, t_in)
            scale = model_fn.guidance_scale
        else:
            e_c, e_u, scale = model_fn(x_eval, torch.full((x.shape[0],), prog['t'][k], device=x.device, dtype=torch.float32)), None, 1.0
        n, slot = prog['nterms'][k], prog['slot'][k]
        if slot >= 0 and hist[slot] is None:
            hist[slot] = torch.empty_like(x)
        acc = _k.dpm_program_step(x_eval, e_c.contiguous(), e_u, scale, prog['conv_x'][k], prog['conv_e'][k], x, hist, slot,
                                  prog['plane'][k][:n], prog['coef'][k][:n])
        x_eval = acc
        if prog['dest'][k] == DEST_STATE:
            x = acc
    return x
