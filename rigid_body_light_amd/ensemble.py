"""Ensembles of independent replicas of one small system (include/rbl.h section 5).

    ens = Ensemble(cfg, X, Q, a, eta, dt, kBT=1.0, wall=True)     # X (R, N_bod, 3), Q (R, N_bod, 4)
    ens.set_interactions(w=0.5, eps_wall=4.0, b_wall=0.1)
    for n in range(steps):
        ens.step_brownian(np.zeros(6), seed=n)                    # every replica, a fixed number of launches
    X, Q = ens.get_config()

All replicas share the structure, the parameters, the wall flag and the force model; each has its own configuration, resident on
the GPU.  Replicas never interact.  Sizes are those of the one-kernel solver (N_bod N_blb <= 256, N_bod <= 64 and its
vectors within 150 KB of LDS, about 75 N_blobs + 60 N_bod doubles: 49 tetrahedra or one body of 238 blobs at max_iter = 255) and
1 <= R <= 65535.
"""
import numpy as np

from ._lib import (McResult,  # noqa: F401  (what metropolis returns)
                   JOINT_BALL, RUN_CHECK_DEFAULT, RUN_REJECT, RUN_STOP, DeviceContext, RblError, blob_anchor, bond_args, cells_args, check_brownian_mask6,
                   default_q_rel, hinge, joint_kind_args, motor, periodic_args, weld)


def _fail(message):
    raise ValueError(message)


class Ensemble:
    def __init__(self, rigid_config, X, Q, a, eta, dt, kBT=1.0, wall=False):
        template = np.asarray(rigid_config, dtype=np.float64)
        if template.size % 3:
            _fail("rigid_config must have length 3 N_blb; got shape %s" % (template.shape,))
        self.blobs_per_body = template.size // 3
        self._cfg = template.reshape(-1, 3).copy()
        self._a = float(a)
        stream = None
        try:
            import torch
            if torch.cuda.is_available():
                stream = torch.cuda.current_stream().cuda_stream
        except ImportError:
            pass
        X, Q = self._shapes(X, Q)
        self.ctx = DeviceContext(a, eta, wall, cfg=template.reshape(-1, 3), dt=dt, kBT=kBT, stream_ptr=stream)
        self.ctx.ensemble_set_config(X, Q)
        self.R, self.N_bodies = X.shape[0], X.shape[1]
        self.last_run = None

    @staticmethod
    def _shapes(X, Q):
        X, Q = np.asarray(X, dtype=np.float64), np.asarray(Q, dtype=np.float64)
        if X.ndim != 3 or X.shape[2] != 3:
            _fail("X must have shape (R, N_bod, 3); got %s" % (X.shape,))
        if Q.ndim != 3 or Q.shape[2] != 4:
            _fail("Q must have shape (R, N_bod, 4); got %s" % (Q.shape,))
        if X.shape[:2] != Q.shape[:2]:
            _fail("X and Q must have the same replicas and bodies; got %s and %s" % (X.shape, Q.shape))
        return X, Q

    def set_config(self, X, Q):
        X, Q = self._shapes(X, Q)
        self.ctx.ensemble_set_config(X, Q)
        self.R, self.N_bodies = X.shape[0], X.shape[1]

    def get_config(self):
        """-> X (R, N_bod, 3), Q (R, N_bod, 4)"""
        return self.ctx.ensemble_get_config()

    def config_dev(self):
        """device addresses of the resident X and Q (for observables computed on the GPU)"""
        return self.ctx.ensemble_config_dev()

    def _forces(self, F):
        F = np.asarray(F, dtype=np.float64)
        per = 6 * self.N_bodies
        if F.shape == (per,):
            return F
        if F.shape == (self.R, per):
            return F
        _fail("F must have shape (%d,) or (%d, %d); got %s" % (per, self.R, per, F.shape))

    def step_deterministic(self, F, max_iter=50, rtol=1e-8, slip=None):
        """one deterministic step of every replica -> (iterations (R,), residual estimates (R,)).  slip: (n3,) or (R, n3)"""
        return self.ctx.ensemble_step_deterministic(self._forces(F), max_iter=max_iter, rtol=rtol, slip=self._slip(slip))

    def step_brownian(self, F, W=None, seed=0, split_rand=True, delta=1e-4, max_iter=50, rtol=1e-8, slip=None):
        """one stochastic midpoint step of every replica -> (iterations (R,), residual estimates (R,)).  W: (R, 9 N_bod N_blb)
        standard normals [W1 | W2 | W_rfd] per replica, or None to draw them from `seed` (replica r from its own counters);
        slip: (n3,) or (R, n3)"""
        F = self._forces(F)
        W = self._noise(W)
        return self.ctx.ensemble_step_brownian(F, W=W, seed=seed, split_rand=split_rand, delta=delta, max_iter=max_iter, rtol=rtol,
                                               slip=self._slip(slip))

    # ------------------------------------------------------------------ prescribed bodies (include/rbl.h sections 5 and 7)
    def _prescribed_mask(self, prescribed):
        """as RigidBody.solve_mixed reads it: a boolean array -- (N_bod,), broadcast over the replicas, or (R, N_bod) -- or a list of
        body indices (integers are ALWAYS indices, the same bodies in every replica) -> uint8 (R, N_bod); ValueError before the
        library is called"""
        p = np.asarray(prescribed)
        R, nb = self.R, self.N_bodies
        if p.dtype == np.bool_:
            if p.shape == (nb,):
                p = np.broadcast_to(p, (R, nb))
            if p.shape != (R, nb):
                _fail("prescribed: a boolean array must have shape (%d,) or (%d, %d); got %s" % (nb, R, nb, p.shape))
            return np.ascontiguousarray(p, dtype=np.uint8)
        if p.size and not np.issubdtype(p.dtype, np.integer):
            _fail("prescribed must be a boolean array or a list of body indices; got dtype %s" % p.dtype)
        idx = p.reshape(-1).astype(np.int64)
        if idx.size and (idx.min() < 0 or idx.max() >= nb):
            _fail("prescribed: body indices must lie in [0, %d)" % nb)
        if np.unique(idx).size != idx.size:
            _fail("prescribed: a body index appears twice (integers are body indices; a 0/1 mask must have dtype bool)")
        mask = np.zeros((R, nb), dtype=np.uint8)
        mask[:, idx] = 1
        return mask

    def _body_in(self, body_in):
        b = np.asarray(body_in, dtype=np.float64)
        R, nb = self.R, self.N_bodies
        if b.shape in ((6 * nb,), (nb, 6)):
            return np.ascontiguousarray(np.broadcast_to(b.reshape(1, 6 * nb), (R, 6 * nb)))
        if b.shape in ((R, 6 * nb), (R, nb, 6)):
            return np.ascontiguousarray(b.reshape(R, 6 * nb))
        _fail("body_in must have shape (%d,), (%d, 6), (%d, %d) or (%d, %d, 6); got %s" % (6 * nb, nb, R, 6 * nb, R, nb, b.shape))

    def _slip(self, slip):
        if slip is None:
            return None
        s = np.asarray(slip, dtype=np.float64)
        n3 = 3 * self.N_bodies * self.blobs_per_body
        if s.shape not in ((n3,), (self.R, n3)):
            _fail("slip must have shape (%d,) or (%d, %d); got %s" % (n3, self.R, n3, s.shape))
        return s

    def _noise(self, W):
        if W is None:
            return None
        W = np.asarray(W, dtype=np.float64)
        n = 9 * self.N_bodies * self.blobs_per_body
        if W.shape != (self.R, n):
            _fail("W must have shape (%d, %d); got %s" % (self.R, n, W.shape))
        return W

    def solve_mixed(self, prescribed, body_in, slip=None, max_iter=100, rtol=1e-8):
        """RigidBody.solve_mixed at every replica's configuration; nothing moves.  The bodies in `prescribed` move with the velocity
        in their six slots of body_in, the others carry their load there.  -> (lambda (R, n3), U (R, 6 N_bod), F (R, 6 N_bod),
        iterations (R,), residual estimates (R,))"""
        m, b, s = self._prescribed_mask(prescribed), self._body_in(body_in), self._slip(slip)
        return self.ctx.ensemble_solve_mixed(m, b, max_iter=max_iter, rtol=rtol, slip=s)

    def step_mixed(self, prescribed, body_in, slip=None, max_iter=50, rtol=1e-8):
        """one deterministic step of every replica with held or driven bodies -> (F (R, 6 N_bod), iterations (R,), residual
        estimates (R,)): a driven body advances by exactly dt U_p, the force model loads the free bodies only"""
        m, b, s = self._prescribed_mask(prescribed), self._body_in(body_in), self._slip(slip)
        return self.ctx.ensemble_step_mixed(m, b, max_iter=max_iter, rtol=rtol, slip=s)

    def step_brownian_mixed(self, prescribed, body_in, slip=None, W=None, seed=0, split_rand=True, delta=1e-4, max_iter=50, rtol=1e-8):
        """one stochastic midpoint step of every replica with held or driven bodies -> (F (R, 6 N_bod), iterations (R,), residual
        estimates (R,)).  F of a prescribed body is its instantaneous load, thermal part included: average it over replicas and
        steps.  W as step_brownian"""
        m, b, s = self._prescribed_mask(prescribed), self._body_in(body_in), self._slip(slip)
        W = self._noise(W)
        return self.ctx.ensemble_step_brownian_mixed(m, b, W=W, seed=seed, split_rand=split_rand, delta=delta, max_iter=max_iter,
                                                     rtol=rtol, slip=s)

    # ------------------------------------------------------------------ prescribed velocity components (the _dof entry points)
    def _prescribed_dof_mask(self, prescribed):
        """as RigidBody.solve_mixed_dof reads it: a boolean array (N_bod, 6) -- translation x, y, z, then rotation x, y, z in the lab
        frame; broadcast over the replicas -- or (R, N_bod, 6) -> uint8 (R, N_bod, 6); ValueError before the library is called.
        Nothing else is read: with R = N_bod = 6 a whole-body mask (R, N_bod) has the shape of (N_bod, 6), hence the separate
        methods and keyword"""
        p = np.asarray(prescribed)
        R, nb = self.R, self.N_bodies
        if p.dtype != np.bool_:
            _fail("prescribed (per component) must be a boolean array; got dtype %s" % p.dtype)
        if p.shape == (nb, 6):
            p = np.broadcast_to(p, (R, nb, 6))
        if p.shape != (R, nb, 6):
            _fail("prescribed (per component) must have shape (%d, 6) or (%d, %d, 6); got %s" % (nb, R, nb, p.shape))
        return np.ascontiguousarray(p, dtype=np.uint8)

    def solve_mixed_dof(self, prescribed, body_in, slip=None, max_iter=100, rtol=1e-8):
        """RigidBody.solve_mixed_dof at every replica's configuration; nothing moves.  prescribed: bool (N_bod, 6) or
        (R, N_bod, 6); a prescribed component moves with its entry of body_in, a free one carries its load there.
        -> (lambda (R, n3), U (R, 6 N_bod), F (R, 6 N_bod), iterations (R,), residual estimates (R,))"""
        m, b, s = self._prescribed_dof_mask(prescribed), self._body_in(body_in), self._slip(slip)
        return self.ctx.ensemble_solve_mixed_dof(m, b, max_iter=max_iter, rtol=rtol, slip=s)

    def step_mixed_dof(self, prescribed, body_in, slip=None, max_iter=50, rtol=1e-8):
        """one deterministic step of every replica with prescribed velocity components -> (F (R, 6 N_bod), iterations (R,),
        residual estimates (R,)): a body with its three translations held keeps X exactly while it turns; the force model loads
        the free components only, so F of a prescribed component is the total load along it"""
        m, b, s = self._prescribed_dof_mask(prescribed), self._body_in(body_in), self._slip(slip)
        return self.ctx.ensemble_step_mixed_dof(m, b, max_iter=max_iter, rtol=rtol, slip=s)

    def step_brownian_mixed_dof(self, prescribed, body_in, slip=None, W=None, seed=0, split_rand=True, delta=1e-4, max_iter=50,
                                rtol=1e-8):
        """one stochastic midpoint step of every replica with prescribed velocity components: a quasi-2D Brownian layer (U_z = 0),
        a trapped probe held in place and free to turn, a roller with Omega imposed whose translation diffuses.  prescribed: bool
        (N_bod, 6) or (R, N_bod, 6) in which every body's three rotation entries are all False or all True -- anything else is a
        ValueError naming the replica and the body: a partly prescribed rotation is not a subset of the coordinates and its drift
        has not been derived.  -> (F (R, 6 N_bod), iterations (R,), residual estimates (R,)); F of a prescribed component is the
        instantaneous load along it, thermal part included.  W as step_brownian"""
        m, b, s = self._prescribed_dof_mask(prescribed), self._body_in(body_in), self._slip(slip)
        check_brownian_mask6("ensemble_step_brownian_mixed_dof", m, self.N_bodies, self.R)
        W = self._noise(W)
        return self.ctx.ensemble_step_brownian_mixed_dof(m, b, W=W, seed=seed, split_rand=split_rand, delta=delta, max_iter=max_iter,
                                                         rtol=rtol, slip=s)

    # ------------------------------------------------------------------ a run of steps (include/rbl.h section 5, rbl_ensemble_run)
    def run(self, n_steps, F=None, prescribed=None, body_in=None, brownian=True, seed=0, stride=0, on_error="stop",
            check_every=RUN_CHECK_DEFAULT, slip=None, split_rand=True, delta=1e-4, max_iter=50, rtol=1e-8, prescribed_dof=None,
            probes=None, probe_body=None, moments=False):
        """n_steps steps of every replica in ONE call: the inputs go to the device once, each step's verdict and commit are taken
        per replica on the device, one read-back ends the run -> RunResult (accepted, rejected, first_status, iters_sum, resid_max,
        F_mean for runs with prescribed bodies, steps_done, stopped_at, and with stride > 0 the frames X, Q, accepted_at, F after
        every stride-th step).  F as step_brownian takes it, or prescribed with body_in as step_brownian_mixed; step n draws its
        noise from seed + n; brownian=False: deterministic steps.  prescribed_dof with body_in (instead of F or prescribed): a mask
        per velocity component as step_mixed_dof takes it, deterministic steps only (a Brownian run at kBT > 0 is refused: loop over
        step_brownian_mixed_dof instead).
        on_error="stop": the first failing step commits nothing, nor does any later one; RblError is raised as the step methods
        raise it, the partial result stays on self.last_run.  on_error="reject": a failing replica keeps its configuration and
        tries again with the next step's noise (the customary redraw, not an unbiased one: see rejected), the others go on; the
        new configuration is validated before it commits; only a failure of the whole batch raises.  check_every: steps between
        the host's looks at the run's status (0: none before the end).
        Observers, evaluated inside every step on that step's blob forces, at the configuration the solve was taken at (q^n, or
        q^{n+1/2} in a Brownian step): probes (P, 3) or (R, P, 3), points at which the fluid velocity is evaluated (velocity_field's
        definition) -- lab points, or with probe_body=b offsets fixed in body b that follow it -- and moments=True for the first
        moments D_b of lambda.  The result gains u_sum / u_mean (R, P, 3) and D_sum / D_mean / stresslet_mean (R, N_bod, 3, 3) over
        the accepted steps and, with stride > 0, frame_u and frame_D.  In a Brownian run these are instantaneous values, thermal
        part included: the mean is the measurement (the drift's share of the stress is not in it)"""
        n_steps, args, obs = self._run_inputs("run", n_steps, F, prescribed, body_in, brownian, seed, stride, on_error, check_every, slip,
                                              split_rand, delta, max_iter, rtol, prescribed_dof, probes, probe_body, moments)
        self.last_run = None
        if obs is None:
            res, rc = self.ctx.ensemble_run(n_steps, **args)
        else:
            res, rc = self.ctx.ensemble_run_observed(n_steps, *obs, **args)
        self.last_run = res
        if rc != 0:
            raise RblError(res.error)
        return res

    def _run_inputs(self, who, n_steps, F, prescribed, body_in, brownian, seed, stride, on_error, check_every, slip, split_rand, delta,
                    max_iter, rtol, prescribed_dof, probes, probe_body, moments):
        """the checks run makes before the library is called, shared with run_driven -> (n_steps, DeviceContext.ensemble_run's
        keywords, the observers or None)"""
        modes = {"stop": RUN_STOP, "reject": RUN_REJECT}
        if on_error not in modes:
            _fail("on_error must be 'stop' or 'reject'; got %r" % (on_error,))
        n_steps, stride, check_every = int(n_steps), int(stride), int(check_every)
        if n_steps < 1:
            _fail("n_steps must be >= 1; got %d" % n_steps)
        if stride < 0 or check_every < 0:
            _fail("stride and check_every must be >= 0; got %d and %d" % (stride, check_every))
        if prescribed_dof is not None and (F is not None or prescribed is not None):
            _fail("prescribed_dof excludes F and prescribed")
        per = 6 if prescribed_dof is not None else 1
        if per == 6:
            if body_in is None:
                _fail("prescribed_dof and body_in go together")
        else:
            if (F is None) == (prescribed is None and body_in is None):
                _fail("give either F or prescribed with body_in")
            if F is None and (prescribed is None or body_in is None):
                _fail("prescribed and body_in go together")
        m = b = None
        if F is not None:
            F = self._forces(F)
        elif per == 6:
            m, b = self._prescribed_dof_mask(prescribed_dof), self._body_in(body_in)
        else:
            m, b = self._prescribed_mask(prescribed), self._body_in(body_in)
        s = self._slip(slip)
        obs = self._observers(who, probes, probe_body, moments)
        args = dict(F_body=F, prescribed=m, body_in=b, brownian=brownian, seed=seed, stride=stride, on_error=modes[on_error],
                    check_every=check_every, slip=s, split_rand=split_rand, delta=delta, max_iter=max_iter, rtol=rtol, per=per)
        return n_steps, args, obs

    # ------------------------------------------------------------------ Metropolis sampling (include/rbl.h section 5, rbl_ensemble_mc)
    def metropolis(self, n_sweeps, step_x, step_theta, seed=0, kBT=None, frozen=None, stride=0, trace=0, sweep_start=0, replica_base=0):
        """n_sweeps Metropolis sweeps of every replica on the total energy of the force model (the one interaction_energy reports),
        in one call: a sweep tries every body once, in order, with a uniform displacement in [-step_x, step_x]^3 and a rotation
        vector in [-step_theta, step_theta]^3 -> McResult (tried, accepted, acceptance, wall_rejected, energy_start, energy_end, and
        with stride > 0 the frames X, Q, E after every stride-th sweep, with trace > 0 the first trials of every replica).  The result
        is the ensemble's configuration: every step continues from it.  kBT: None (the ensemble's), one value, or (R,) for a
        temperature sweep; frozen: (N_bod,) or (R, N_bod), bodies that never move and still act on the others.  The draws depend on
        (seed, replica_base + r, sweep_start + s, b) alone: n1 + n2 sweeps are n1 sweeps followed by n2 with sweep_start=n1, and
        replica r is a one-replica ensemble with replica_base=r.  Not offered: dipole terms, hard joints, moves of several bodies,
        cluster or swap moves, replica exchange (RblError names the term)"""
        return self.ctx.ensemble_mc(n_sweeps, step_x, step_theta, seed=seed, kBT=kBT, frozen=frozen, stride=stride, trace=trace,
                                    sweep_start=sweep_start, replica_base=replica_base)   # (the binding owns the argument checks)

    def metropolis_tune(self, target=0.4, n_sweeps=20, rounds=8, step_x=0.1, step_theta=0.1, seed=0, kBT=None, frozen=None):
        """a host loop that scales BOTH step sizes by one common factor towards the acceptance `target` (mean over the replicas):
        `rounds` chains of n_sweeps sweeps, each followed by factor = clip(acceptance / target, 0.5, 2) -> (step_x, step_theta).
        The chains move the ensemble (a burn-in).  Adapting the steps while sampling would bias the chain: tune first, then
        sample with the returned steps held fixed"""
        if not 0.0 < target < 1.0:
            _fail("metropolis_tune: target must lie in (0, 1); got %r" % (target,))
        if int(rounds) < 1:
            _fail("metropolis_tune: rounds must be >= 1; got %r" % (rounds,))
        sx, st = float(step_x), float(step_theta)
        for k in range(int(rounds)):
            res = self.metropolis(n_sweeps, sx, st, seed=seed, kBT=kBT, frozen=frozen, sweep_start=k * int(n_sweeps))
            acc = float(res.accepted.sum()) / max(1, int(res.tried.sum()))
            f = min(2.0, max(0.5, acc / target))
            sx, st = sx * f, st * f
        return sx, st

    # ------------------------------------------------------------------ driven runs (include/rbl.h section 5, rbl_ensemble_run_driven)
    def _drive(self, who, cos, sin, omega, t0, schedule, cycle_start, lockin=False):
        """the drive's arrays as run_driven and drive_eval take them -> DeviceContext.ensemble_run_driven's keywords; ValueError
        before the library is called.  cos, sin: (6 N_bod,), (N_bod, 6), or either with a leading R; omega, t0: a number or (R,);
        schedule = (phase_steps, phase_in), phase_in (n_phases, 6 N_bod) or (n_phases, R, 6 N_bod); cycle_start an integer or (R,)"""
        R, nb6 = self.R, 6 * self.N_bodies
        d = dict(lockin=bool(lockin))
        for name, a in (("cos", cos), ("sin", sin)):
            if a is None:
                continue
            a = np.asarray(a, dtype=np.float64)
            if a.shape in ((nb6,), (self.N_bodies, 6)):
                a = a.reshape(1, nb6)
            elif a.shape in ((R, nb6), (R, self.N_bodies, 6)):
                a = a.reshape(R, nb6)
            else:
                _fail("%s: %s must have shape (%d,), (%d, 6), (%d, %d) or (%d, %d, 6); got %s"
                      % (who, name, nb6, self.N_bodies, R, nb6, R, self.N_bodies, a.shape))
            if not np.isfinite(a).all():
                _fail("%s: %s must be finite" % (who, name))
            d[name] = np.ascontiguousarray(a)
        harmonic = "cos" in d or "sin" in d
        for name, a in (("omega", omega), ("t0", t0)):
            if a is None:
                continue
            a = np.asarray(a, dtype=np.float64)
            if a.shape not in ((), (1,), (R,)):
                _fail("%s: %s must be a number or have shape (%d,); got %s" % (who, name, R, a.shape))
            if not np.isfinite(a).all():
                _fail("%s: %s must be finite" % (who, name))
            d[name] = a.reshape(-1)
        if (harmonic or lockin) and "omega" not in d:
            _fail("%s: omega is needed with cos, sin or lockin" % who)
        length = 0
        if schedule is not None:
            try:
                ps, pi = schedule
            except (TypeError, ValueError):
                _fail("%s: schedule must be a pair (phase_steps, phase_in)" % who)
            ps, pi = np.asarray(ps), np.asarray(pi, dtype=np.float64)
            if ps.ndim != 1 or not ps.size or not np.issubdtype(ps.dtype, np.integer):
                _fail("%s: phase_steps must be a non-empty list of integers; got shape %s, dtype %s" % (who, ps.shape, ps.dtype))
            if (ps < 1).any():
                _fail("%s: phase_steps[%d] = %d: every phase lasts at least one step" % (who, int(np.flatnonzero(ps < 1)[0]), int(ps[ps < 1][0])))
            length = int(ps.astype(np.int64).sum())
            if length > 2**31 - 1:
                _fail("%s: the cycle's length (the sum of phase_steps) must fit 31 bits" % who)
            if pi.shape not in ((ps.size, nb6), (ps.size, R, nb6)):
                _fail("%s: phase_in: one input per phase, shape (%d, %d) or (%d, %d, %d); got %s" % (who, ps.size, nb6, ps.size, R, nb6, pi.shape))
            if not np.isfinite(pi).all():
                _fail("%s: phase_in must be finite" % who)
            d["phase_steps"], d["phase_in"] = ps.astype(np.int32), np.ascontiguousarray(pi)
        if cycle_start is not None:
            cs = np.asarray(cycle_start)
            if cs.shape not in ((), (1,), (R,)) or not np.issubdtype(cs.dtype, np.integer):
                _fail("%s: cycle_start must be an integer or %d integers; got shape %s, dtype %s" % (who, R, cs.shape, cs.dtype))
            cs = cs.reshape(-1)
            if (cs < 0).any() or (cs >= max(length, 1)).any():
                _fail("%s: cycle_start must lie in the cycle, 0 <= value < %d; got %s" % (who, max(length, 1), cs.tolist()))
            d["cycle_start"] = cs.astype(np.int32)
        return d

    def run_driven(self, n_steps, F=None, prescribed=None, body_in=None, cos=None, sin=None, omega=0.0, t0=None, schedule=None,
                   cycle_start=None, lockin=False, brownian=True, seed=0, stride=0, on_error="stop", check_every=RUN_CHECK_DEFAULT,
                   slip=None, split_rand=True, delta=1e-4, max_iter=50, rtol=1e-8, prescribed_dof=None, probes=None, probe_body=None,
                   moments=False):
        """run with a body input that follows a drive, in ONE call (rbl_ensemble_run_driven): before every step replica r steps with
            ((A0 + P[phase(p_r)]) + cos * cs) + sin * sn,    cs, sn = cos, sin(omega_r t_r),    t_r = t0_r + dt * accepted_r
        where A0 is F (all bodies free) or body_in (with prescribed / prescribed_dof: velocities on prescribed entries, loads on
        free ones).  cos, sin: amplitudes (6 N_bod,) / (N_bod, 6), or with a leading R one set per replica; omega: a number or
        (R,) -- one frequency per replica makes the run a spectrum --; t0: a number or (R,), None: 0.  schedule = (phase_steps,
        phase_in): a periodic piecewise-constant part, phase k lasting phase_steps[k] steps with phase_in[k] ((n_phases, 6 N_bod)
        or (n_phases, R, 6 N_bod)), on the replica's own cycle position, which starts at cycle_start and moves on when the replica
        commits; a rejected replica's clock and position wait for it.  lockin=True: the result carries X_c, X_s, U_c, U_s, F_c,
        F_s and norm (RunResult).  It always carries cycle_pos and t_end: run_driven(..., cycle_start=res.cycle_pos, t0=res.t_end)
        continues the run.  The run is bit for bit the loop of drive_eval and the one-step method; with no drive it is run().
        The remaining keywords are run's.  Hard joints switched on: RblError (a drive with joints is not offered)"""
        n_steps, args, obs = self._run_inputs("run_driven", n_steps, F, prescribed, body_in, brownian, seed, stride, on_error, check_every,
                                              slip, split_rand, delta, max_iter, rtol, prescribed_dof, probes, probe_body, moments)
        drive = self._drive("run_driven", cos, sin, omega, t0, schedule, cycle_start, lockin)
        if obs is not None:
            args.update(probes=obs[0], probe_body=obs[1], moments=obs[2])
        self.last_run = None
        res, rc = self.ctx.ensemble_run_driven(n_steps, **drive, **args)
        self.last_run = res
        if rc != 0:
            raise RblError(res.error)
        return res

    def drive_eval(self, base, accepted=None, cycle_pos=None, cos=None, sin=None, omega=0.0, t0=None, schedule=None, cycle_start=None):
        """the body input run_driven's kernel gives a step that starts with the counters accepted (R,) (None: zeros) and the cycle
        positions cycle_pos (R,) (None: cycle_start) -> (input (R, 6 N_bod), cs_sn (R, 2)).  base: A0, as F or body_in.  One
        launch of the run's own kernel: hand the input to step_deterministic, step_brownian(seed + n), step_mixed, ... and the
        loop reproduces the run bit for bit (numpy's cos and sin are not the device's)"""
        A0 = self._body_in(base)
        drive = self._drive("drive_eval", cos, sin, omega, t0, schedule, cycle_start)
        drive.pop("lockin")
        ints = []
        for name, a in (("accepted", accepted), ("cycle_pos", cycle_pos)):
            if a is not None:
                a = np.asarray(a)
                if a.shape != (self.R,) or not np.issubdtype(a.dtype, np.integer):
                    _fail("drive_eval: %s must be %d integers; got shape %s, dtype %s" % (name, self.R, a.shape, a.dtype))
                if (a < 0).any():
                    _fail("drive_eval: %s must be >= 0" % name)
            ints.append(a)
        return self.ctx.ensemble_drive_eval(A0, accepted=ints[0], cycle_pos=ints[1], **drive)

    # ------------------------------------------------------------------ the flow at probe points, observers (include/rbl.h section 5)
    def _points(self, who, points):
        """(P, 3), one set of points for every replica, or (R, P, 3); finite -> a contiguous float64 array; ValueError before the
        library is called"""
        p = np.asarray(points, dtype=np.float64)
        if p.shape[-1:] != (3,) or not (p.ndim == 2 or (p.ndim == 3 and p.shape[0] == self.R)):
            _fail("%s: points must have shape (P, 3) or (%d, P, 3); got %s" % (who, self.R, p.shape))
        bad = np.argwhere(~np.isfinite(p).all(axis=-1))
        if bad.size:
            _fail("%s: points: %spoint %d has a non-finite coordinate" % (who, "set %d, " % bad[0][0] if p.ndim == 3 else "", bad[0][-1]))
        return np.ascontiguousarray(p)

    def _probe_body(self, who, body):
        if body is None:
            return None
        if isinstance(body, bool) or int(body) != body or not 0 <= int(body) < self.N_bodies:
            _fail("%s: the probes' body must be None (lab points) or a body index in [0, %d); got %r" % (who, self.N_bodies, body))
        return int(body)

    def _observers(self, who, probes, probe_body, moments):
        """-> None when nothing is observed (the run is then today's call), else (points or None, body or None, moments)"""
        if probes is None and probe_body is None and not moments:
            return None
        if probes is None and probe_body is not None:
            _fail("%s: probe_body was given without probes" % who)
        pts = None if probes is None else self._points(who, probes)
        return pts, self._probe_body(who, probe_body), bool(moments)

    def velocity_field(self, points, lam, body=None):
        """the fluid velocity every replica's blob forces drive at points, at the ensemble's current configuration and in its cell
        (set_cell) -> (R, P, 3).  points: (P, 3), shared by the replicas, or (R, P, 3); lam: (R, 3 N), e.g. solve_jointed's or
        solve_mixed's lambda.  The velocity apply_M would give a force-free blob of radius a placed there: a point on a blob
        returns that blob's row, with the wall a point at z <= 0 gets 0.  body=b: the points are offsets fixed in body b of each
        replica, placed at X_b + R(Q_b) s; the velocity stays in lab-frame components"""
        pts = self._points("velocity_field", points)
        lam = np.asarray(lam, dtype=np.float64)
        n3 = 3 * self.N_bodies * self.blobs_per_body
        if lam.shape != (self.R, n3):
            _fail("velocity_field: lam must have shape (%d, %d); got %s" % (self.R, n3, lam.shape))
        return self.ctx.ensemble_velocity_field(pts, lam, body=self._probe_body("velocity_field", body))

    def probe_info(self, n_points):
        """(points per lane, waves per workgroup, point tiles) of the probe kernel's launch for n_points points per replica"""
        return self.ctx.ensemble_probe_info(int(n_points))

    def body_resistance_matrix(self, max_iter=100, rtol=1e-8):
        """the body resistance matrix of every replica's configuration, (R, 6 N_bod, 6 N_bod): every body prescribed, one ensemble
        solve per unit velocity; sign as RigidBody.body_resistance_matrix (a column is -F: the PHYSICAL loads R U, nothing
        is symmetrised)"""
        nb6 = 6 * self.N_bodies
        everyone = np.ones((self.R, self.N_bodies), dtype=bool)
        Rm = np.zeros((self.R, nb6, nb6))
        for j in range(nb6):
            U = np.zeros(nb6)
            U[j] = 1.0
            Rm[:, :, j] = -self.solve_mixed(everyone, U, max_iter=max_iter, rtol=rtol)[2]
        return Rm

    def set_interactions(self, w=0.0, eps_wall=0.0, b_wall=1.0, eps_blob=0.0, b_blob=1.0, r_cut=None, on=True):
        """the force model of RigidBody.set_interactions, for every replica (steric pairs only inside a replica)"""
        self.ctx.set_interactions(w=w, eps_wall=eps_wall, b_wall=b_wall, eps_blob=eps_blob, b_blob=b_blob, r_cut=r_cut, on=on)

    def set_pair_table(self, U, dU, r_min, r_cut, on=True):
        """the tabulated pair potential of RigidBody.set_pair_table, for every replica (pairs only inside a replica)"""
        self.ctx.set_pair_table(U, dU, r_min, r_cut, on=on)

    def set_height_table(self, U, dU, h_min, h_cut, on=True):
        """the tabulated potential in the blob height of RigidBody.set_height_table, for every replica"""
        self.ctx.set_height_table(U, dU, h_min, h_cut, on=on)

    def set_blob_types(self, types, n_types=None, on=True):
        """the blob types of RigidBody.set_blob_types: (N_blb,) -- every body alike -- or (N_bod, N_blb), the system of ONE
        replica, shared by every replica"""
        if types is None and not on:
            return self.ctx.set_blob_types(None, on=False)
        t = np.asarray(types)
        if t.shape not in ((self.blobs_per_body,), (self.N_bodies, self.blobs_per_body)):
            _fail("types must have shape (%d,) or (%d, %d); got %s" % (self.blobs_per_body, self.N_bodies, self.blobs_per_body, t.shape))
        self.ctx.set_blob_types(t, n_types=n_types, on=on)

    def blob_types(self):
        return self.ctx.blob_types()

    def set_type_table(self, ta, tb, U, dU, r_min, r_cut, on=True):
        """the table of the type pair (ta, tb) of RigidBody.set_type_table, for every replica (pairs only inside a replica)"""
        self.ctx.set_type_table(ta, tb, U, dU, r_min, r_cut, on=on)

    def type_table(self, ta, tb):
        return self.ctx.type_table(ta, tb)

    def clear_type_tables(self):
        self.ctx.clear_type_tables()

    def set_traps(self, k, X0, on=True):
        """harmonic traps on the body centres: k and X0 of shape (N_bod, 3), shared by every replica, or (R, N_bod, 3)"""
        k, X0 = np.asarray(k, dtype=np.float64), np.asarray(X0, dtype=np.float64)
        nb = self.N_bodies
        if k.shape != X0.shape or k.shape not in ((nb, 3), (self.R, nb, 3)):
            _fail("k and X0 must both have shape (%d, 3) or (%d, %d, 3); got %s and %s" % (nb, self.R, nb, k.shape, X0.shape))
        self.ctx.set_traps(k.reshape(-1, 3), X0.reshape(-1, 3), on=on)

    def set_dipoles(self, m_body, c_dd=0.0, r_core=None, r_cut=np.inf, on=True):
        """the permanent moments of RigidBody.set_dipoles: m_body of shape (3,) -- every body of every replica alike --,
        (N_bod, 3), shared by every replica, or (R, N_bod, 3); dipole pairs only inside a replica"""
        if m_body is None and not on:
            return self.ctx.set_dipoles(None, on=False)
        m = np.asarray(m_body, dtype=np.float64)
        nb = self.N_bodies
        if m.shape not in ((3,), (nb, 3), (self.R, nb, 3)):
            _fail("m_body must have shape (3,), (%d, 3) or (%d, %d, 3); got %s" % (nb, self.R, nb, m.shape))
        self.ctx.set_dipoles(m.reshape(-1, 3), c_dd=c_dd, r_core=r_core, r_cut=r_cut, on=on)

    def dipoles(self):
        return self.ctx.dipoles()

    def set_magnetic_field(self, B0=None, B1=None, B2=None, omega=0.0, on=True):
        """the uniform field of RigidBody.set_magnetic_field, one for all replicas"""
        self.ctx.set_magnetic_field(B0, B1, B2, omega=omega, on=on)

    def magnetic_field(self):
        return self.ctx.magnetic_field()

    def set_field_time(self, t):
        """the field's clock: a number for all replicas or (R,), one per replica.  The one-step methods evaluate the field at
        this time and do not advance it.  run() evaluates step by step at t[r] + dt * (replica r's accepted steps so far) and
        leaves the value set here as it was: continue with t + dt * result.accepted"""
        t = np.asarray(t, dtype=np.float64)
        if t.shape not in ((), (1,), (self.R,)):
            _fail("t must be a number or have shape (%d,); got %s" % (self.R, t.shape))
        self.ctx.set_field_time(t)

    def field_time(self):
        return self.ctx.field_time()

    def set_bonds(self, body, anchor_a, anchor_b, k, l0=0.0, kind=None, on=True):
        """the bonds and tethers of RigidBody.set_bonds, for every replica: the topology (body, kind) and the anchors are shared,
        indices are local to a replica and replicas never bond to each other.  k, l0: a number or (n_bonds,), shared, or
        (R, n_bonds): a stiffness or rest-length sweep with one set per replica"""
        if body is None and not on:
            return self.ctx.set_bonds(None, None, None, None, on=False)
        b, anchor, kind, param = bond_args("set_bonds", body, anchor_a, anchor_b, k, l0, kind, sets=(1, self.R))
        self.ctx.set_bonds(b, anchor[:, :3], anchor[:, 3:], param[:, :, 0], param[:, :, 1], kind=kind, on=on)

    def bonds(self):
        return self.ctx.bonds()

    def set_joints(self, *args, **kwargs):
        """RigidBody.set_joints is not offered for ensembles under that name: an ensemble's hard joints of every kind, ball joints
        included, are stored by set_joint_kinds (kind=None: all ball joints) and act in solve_jointed / step_jointed"""
        raise ValueError("set_joints: not offered for ensembles (include/rbl.h section 5): use set_joint_kinds -- kind=None stores ball "
                         "joints -- with solve_jointed / step_jointed")

    # ------------------------------------------------------------------ hard joints (include/rbl.h sections 5 and 9)
    def set_joint_kinds(self, body, kind, anchor_a=None, anchor_b=None, axis=None, q_rel=None, on=True):
        """the joints of RigidBody.set_joint_kinds for every replica: topology, kinds, anchors, axes and q_rel are shared, body
        indices are local to a replica.  kind=None: all ball joints.  q_rel=None: Q_A^-1 Q_B of replica 0's configuration.
        They act in solve_jointed / step_jointed only.  body=None with on=False only switches them off"""
        if body is None:
            if on:
                _fail("set_joint_kinds: body is None: that only switches the stored joints off, with on=False")
            return self.ctx.set_joint_kinds(None, None, on=False)
        if kind is None:
            kind = np.zeros(np.asarray(body).reshape(-1, 2).shape[0], dtype=np.int32)
        b, k, anchor, ax, qr = joint_kind_args("set_joint_kinds", body, kind, anchor_a, anchor_b, axis, q_rel)
        if b.max() >= self.N_bodies:
            _fail("set_joint_kinds: body indices are local to a replica and must lie below %d" % self.N_bodies)
        if q_rel is None and (k != JOINT_BALL).any():
            default_q_rel("set_joint_kinds", b, k, qr, self.get_config()[1][0])
        self.ctx.set_joint_kinds(b, k, anchor[:, :3], anchor[:, 3:], axis=ax, q_rel=qr, on=on)

    def joint_kinds(self):
        """{on, by_kinds, body, anchor_a, anchor_b, kind, axis, q_rel, theta (R, n_joints)} of the stored joints.  The motors' rates
        are not among them: an ensemble's are per replica and the library does not hand them back (keep what set_joint_rates got)"""
        d = self.ctx.joint_kinds()
        d.pop("rate")                                      # (the single context's own rates, which an ensemble does not use)
        d["theta"] = self.ctx.ensemble_joint_state(phi=False)[2] if d["kind"].shape[0] else np.zeros((self.R, 0))
        return d

    def _joint_values(self, who, v):
        n = self.ctx.joints()["body"].shape[0]           # (a host-side query: the stored set is the context's, whoever stored it)
        v = np.asarray(v, dtype=np.float64)
        if not n or v.shape not in ((n,), (self.R, n)):
            _fail("%s: one value per stored joint, shape (%d,) or (%d, %d); got %s" % (who, n, self.R, n, v.shape))
        return v

    def set_joint_rates(self, rates):
        """the motors' rates: (n_joints,) shared by the replicas, or (R, n_joints), one set per replica; non-zero on lock joints only"""
        rates = self._joint_values("set_joint_rates", rates)
        self.ctx.ensemble_set_joint_rates(rates)

    def set_joint_angles(self, theta):
        """the motors' angles: (n_joints,) or (R, n_joints): a sweep of stroke phases, or a restart"""
        theta = self._joint_values("set_joint_angles", theta)
        self.ctx.ensemble_set_joint_angles(theta)

    def _joint_rows_in(self, who, v, n):
        """joint_rhs / joint_velocity: (3 n,), (n, 3), or either with a leading R -> (R, 3 n) or (3 n,)"""
        if v is None:
            return None
        v = np.asarray(v, dtype=np.float64)
        if v.shape in ((3 * n,), (n, 3)):
            return v.reshape(3 * n)
        if v.shape in ((self.R, 3 * n), (self.R, n, 3)):
            return np.ascontiguousarray(v.reshape(self.R, 3 * n))
        _fail("%s must have shape (%d,), (%d, 3), (%d, %d) or (%d, %d, 3); got %s" % (who, 3 * n, n, self.R, 3 * n, self.R, n, v.shape))

    def _joints_on(self):
        d = self.ctx.joints()                              # (a host-side query: the stored set is the context's, whoever stored it)
        return d["body"].shape[0] if d["on"] else 0

    def solve_jointed(self, F, slip=None, joint_rhs=None, max_iter=100, rtol=1e-8):
        """RigidBody.solve_jointed at every replica's configuration in one solver launch; nothing moves -> (lambda (R, n3),
        U (R, 6 N_bod), phi (R, 3 n_joints), iterations (R,), residual estimates (R,)).  Joints off or never set: the unjointed
        solve, phi empty"""
        F, s = self._forces(F), self._slip(slip)
        jr = self._joint_rows_in("joint_rhs", joint_rhs, self._joints_on())
        return self.ctx.ensemble_solve_jointed(F, slip=s, joint_rhs=jr, max_iter=max_iter, rtol=rtol)

    def step_jointed(self, F, slip=None, joint_velocity=None, gamma=1.0, max_iter=50, rtol=1e-8):
        """one deterministic step of every replica with the joints, J U = -(gamma / dt) gap + joint_velocity - rate ah (a motor's
        rows), in one solver launch -> (phi (R, 3 n_joints), iterations (R,), residual estimates (R,)).  The first failing replica
        raises and nothing moves; every motor's angle advances by rate dt when the step commits"""
        F, s = self._forces(F), self._slip(slip)
        jv = self._joint_rows_in("joint_velocity", joint_velocity, self._joints_on())
        return self.ctx.ensemble_step_jointed(F, slip=s, joint_velocity=jv, gamma=gamma, max_iter=max_iter, rtol=rtol)

    def _schedule(self, schedule, cycle_start):
        """(phase_steps, phase_rates) and the starting positions as run_jointed takes them -> (int32 (n_phases,), float64
        (n_phases, n_joints) or (n_phases, R, n_joints), int32 (1,) or (R,)), each None where not given; ValueError before the
        library is called"""
        ps = pr = cs = None
        length = 0
        if schedule is not None:
            n = self.ctx.joints()["body"].shape[0]
            try:
                ps, pr = schedule
            except (TypeError, ValueError):
                _fail("run_jointed: schedule must be a pair (phase_steps, phase_rates)")
            ps, pr = np.asarray(ps), np.asarray(pr, dtype=np.float64)
            if ps.ndim != 1 or not ps.size or not np.issubdtype(ps.dtype, np.integer):
                _fail("run_jointed: phase_steps must be a non-empty list of integers; got shape %s, dtype %s" % (ps.shape, ps.dtype))
            if (ps < 1).any():
                _fail("run_jointed: phase_steps[%d] = %d: every phase lasts at least one step" % (int(np.flatnonzero(ps < 1)[0]), int(ps[ps < 1][0])))
            length = int(ps.astype(np.int64).sum())
            if length > 2**31 - 1:
                _fail("run_jointed: the cycle's length (the sum of phase_steps) must fit 31 bits")
            if not n or pr.shape not in ((ps.size, n), (ps.size, self.R, n)):
                _fail("run_jointed: phase_rates: one rate per phase and stored joint, shape (%d, %d) or (%d, %d, %d); got %s"
                      % (ps.size, n, ps.size, self.R, n, pr.shape))
            if not np.isfinite(pr).all():
                _fail("run_jointed: phase_rates must be finite")
            ps = ps.astype(np.int32)
        if cycle_start is not None:
            cs = np.asarray(cycle_start)
            if cs.shape not in ((), (1,), (self.R,)) or not np.issubdtype(cs.dtype, np.integer):
                _fail("run_jointed: cycle_start must be an integer or %d integers; got shape %s, dtype %s" % (self.R, cs.shape, cs.dtype))
            cs = cs.reshape(-1)
            if (cs < 0).any() or (cs >= max(length, 1)).any():
                _fail("run_jointed: cycle_start must lie in the cycle, 0 <= value < %d; got %s" % (max(length, 1), cs.tolist()))
            cs = cs.astype(np.int32)
        return ps, pr, cs

    def run_jointed(self, n_steps, F, slip=None, joint_velocity=None, gamma=1.0, schedule=None, cycle_start=None, stride=0,
                    on_error="stop", check_every=RUN_CHECK_DEFAULT, max_iter=50, rtol=1e-8, probes=None, probe_body=None, moments=False):
        """n_steps steps of step_jointed in ONE call (rbl_ensemble_run_jointed): the joint table, F, slip and joint_velocity go to
        the device once, the motors' angles advance there, one read-back ends the run -> RunResult, with theta (R, n_joints) and
        cycle_pos (R,) as the run leaves them, phi_sum / phi_mean (R, n_joints, 3) over the accepted steps (a motor's mean torque
        is phi_mean of its lock rows) and, with stride > 0, the frames X, Q, accepted_at, frame_theta, frame_phi (the step's phi,
        or the last accepted one) and frame_gap (joint_state's gaps at the committed configuration).
        schedule = (phase_steps, phase_rates): a periodic, piecewise-constant motor schedule, phase k lasting phase_steps[k] steps
        with the rates phase_rates[k] -- (n_phases, n_joints), or (n_phases, R, n_joints) for rates per replica; non-zero on motors
        only --, evaluated on each replica's own position in the cycle, which starts at cycle_start (an integer or (R,); 0 when
        None) and moves on when the replica commits.  cycle_start=res.cycle_pos continues a stroke.  schedule=None: the rates of
        set_joint_rates, constant; set_joint_rates' rates are untouched by a schedule.  on_error and check_every as in run; a
        stopped run raises RblError and leaves the partial result on self.last_run.  Joints off or never set: run(brownian=False).
        probes, probe_body and moments: the observers of run, evaluated at q^n of every step; probes fixed in a link
        (probe_body) give the flow in the swimmer's frame of reference, still in lab-frame components"""
        modes = {"stop": RUN_STOP, "reject": RUN_REJECT}
        if on_error not in modes:
            _fail("on_error must be 'stop' or 'reject'; got %r" % (on_error,))
        n_steps, stride, check_every = int(n_steps), int(stride), int(check_every)
        if n_steps < 1:
            _fail("n_steps must be >= 1; got %d" % n_steps)
        if stride < 0 or check_every < 0:
            _fail("stride and check_every must be >= 0; got %d and %d" % (stride, check_every))
        if not 0.0 <= float(gamma) <= 1.0:
            _fail("gamma must lie in [0, 1]; got %r" % (gamma,))
        F, s = self._forces(F), self._slip(slip)
        jv = self._joint_rows_in("joint_velocity", joint_velocity, self._joints_on())
        ps, pr, cs = self._schedule(schedule, cycle_start)
        obs = self._observers("run_jointed", probes, probe_body, moments)
        self.last_run = None
        args = dict(slip=s, joint_velocity=jv, gamma=gamma, phase_steps=ps, phase_rates=pr, cycle_start=cs, stride=stride,
                    on_error=modes[on_error], check_every=check_every, max_iter=max_iter, rtol=rtol)
        if obs is None:
            res, rc = self.ctx.ensemble_run_jointed(n_steps, F, **args)
        else:
            res, rc = self.ctx.ensemble_run_observed(n_steps, *obs, jointed=True, F_body=F, **args)
        self.last_run = res
        if rc != 0:
            raise RblError(res.error)
        return res

    def joint_state(self, phi=True):
        """-> (gap (R, n_joints, 3) at the current configurations, phi (R, n_joints, 3) of the last jointed solve or step,
        theta (R, n_joints)).  phi=False leaves phi out (None): the query then also serves before any jointed solve"""
        return self.ctx.ensemble_joint_state(phi=phi)

    def _replica_config(self, replica):
        X, Q = self.get_config()
        if not 0 <= int(replica) < self.R:
            _fail("replica must lie in [0, %d); got %r" % (self.R, replica))
        return X[int(replica)], Q[int(replica)]

    def hinge(self, a, b, point, axis, replica=0):
        """rows of a five-row hinge (ball + axis joint) for joint_rows / set_joint_kinds: point and axis in the lab frame, the
        body-frame anchors, axis and q_rel taken from the named replica's configuration"""
        return hinge(*self._replica_config(replica), a, b, point, axis)

    def weld(self, a, b, point, replica=0):
        """rows of a weld (ball + lock joint) at the named replica's configuration"""
        return weld(*self._replica_config(replica), a, b, point)

    def motor(self, a, b, point, axis, replica=0):
        """rows of a motor (ball + lock joint, driven by set_joint_rates) at the named replica's configuration"""
        return motor(*self._replica_config(replica), a, b, point, axis)

    def set_periodic(self, *args, **kwargs):
        """the single context's cell (RigidBody.set_periodic) is not offered for ensembles under that name: an ensemble's cell is
        state of its own, stored by set_cell"""
        raise ValueError("set_periodic: a periodic cell is not offered for ensembles under this name (include/rbl.h section 10): "
                         "use set_cell (rbl_ensemble_set_periodic, section 5)")

    # ------------------------------------------------------------------ periodic cell in x and y (include/rbl.h sections 5 and 10)
    def set_cell(self, Lx, Ly, images=(1, 1), on=True):
        """One periodic cell of lengths Lx, Ly (0: that axis stays open) shared by all replicas: the one-kernel solver's operator,
        the drift and the dense Brownian root sum every pair over images = (nx, ny) periodic images on either side of its nearest
        one (1 <= n <= 16 on a periodic axis), a blob's own images included, and the pair forces use the minimum image.  Needs
        the wall; L must exceed 4a.  Coordinates stay unwrapped.  Every step, solve and run takes the cell; solve_jointed,
        step_jointed, run_jointed and joint_state are refused (RblError, "periodic") while it is on.  on=False stores it switched off."""
        Lx, Ly, nx, ny = periodic_args("set_cell", Lx, Ly, images)
        self.ctx.ensemble_set_periodic(Lx, Ly, images=(nx, ny), on=bool(on))

    def cell(self):
        """-> {Lx, Ly, images, on} of the ensemble's cell; raises while a cell per replica is stored (see cells)"""
        try:
            return self.ctx.ensemble_periodic()
        except RblError as e:
            if self.ctx.ensemble_cells()["per_replica"]:
                raise RblError("cell: the ensemble holds a cell per replica, there is no one cell to report: use cells() (%s)" % e) from None
            raise

    def set_cells(self, Lx, Ly, images=(1, 1), on=True):
        """A periodic cell PER REPLICA -- an area-fraction sweep, or a convergence study in the image count, in one call.  Lx, Ly:
        real scalars or (R,); images: (nx, ny) or (R, 2); scalars broadcast.  Replica r is what an R = 1 ensemble gives after
        set_cell(Lx[r], Ly[r], images[r]), bit for bit; a replica may keep an axis open (L = 0) while another has it periodic.  A
        replica with more images runs more steps of the pair sweep, and a launch lasts as long as its slowest replica.  Replaces
        the shared cell of set_cell, as set_cell replaces this.  The cells belong to this R."""
        Lx, Ly, n = cells_args("set_cells", Lx, Ly, images, self.R)
        self.ctx.ensemble_set_cells(Lx, Ly, images=n, on=bool(on))

    def cells(self):
        """-> {on, per_replica, Lx (R,), Ly (R,), images (R, 2)}: the cell of every replica (a shared cell: R equal rows)"""
        return self.ctx.ensemble_cells()

    def area_fraction(self, body_area):
        """(R,) N_bod body_area / (Lx Ly) of every replica, the label of an area-fraction sweep (body_area: the area one body
        covers, e.g. pi R_h^2); nan for a replica that is not periodic in both axes.  No device work"""
        c = self.cells()
        A = c["Lx"] * c["Ly"]
        out = np.full(self.R, np.nan)
        ok = (c["Lx"] > 0.0) & (c["Ly"] > 0.0)
        out[ok] = self.N_bodies * float(body_area) / A[ok]
        return out

    def set_bond_table(self, U, dU, r_min, r_cut, on=True):
        """the potential of the kind-1 bonds of RigidBody.set_bond_table, one for all replicas"""
        self.ctx.set_bond_table(U, dU, r_min, r_cut, on=on)

    def bond_state(self):
        """-> (length, tension dU/dd, energy) of every bond of every replica, (R, n_bonds) each"""
        return self.ctx.ensemble_bond_state()

    def blob_anchor(self, k):
        """body-frame position of blob k with the structure's mean removed: the anchor of a bond that ends on that blob"""
        return blob_anchor(self._cfg, k)

    def interaction_forces(self):
        """body forces and torques of the model, (R, 6 N_bod), reference convention (-K^T f_phys)"""
        return self.ctx.ensemble_interaction_forces()[0]

    def interaction_energy(self):
        """total potential energy of every replica, (R,)"""
        return self.ctx.ensemble_interaction_forces()[1]

    # ------------------------------------------------------------------ imposed flow, active slip, stresslets (include/rbl.h section 8)
    def set_background_flow(self, u0=None, G=None, on=True):
        """the background flow of RigidBody.set_background_flow, one for all replicas: every step adds -(u0 + G r) at the blobs of
        q^n to its slip, in one launch over all replicas"""
        u0 = np.zeros(3) if u0 is None else np.asarray(u0, dtype=np.float64)
        G = np.zeros((3, 3)) if G is None else np.asarray(G, dtype=np.float64)
        if u0.shape != (3,):
            _fail("u0 must have shape (3,); got %s" % (u0.shape,))
        if G.shape != (3, 3):
            _fail("G must have shape (3, 3); got %s" % (G.shape,))
        self.ctx.set_background_flow(u0, G, on=on)

    def set_body_slip(self, slip_body, scale=None, on=True):
        """the body-frame slip pattern of RigidBody.set_body_slip; scale (N_bod,): scale[b] serves body b of every replica"""
        sb = np.asarray(slip_body, dtype=np.float64)
        if sb.size != 3 * self.blobs_per_body or not (sb.ndim == 1 or (sb.ndim == 2 and sb.shape[1] == 3)):
            _fail("slip_body must have shape (%d, 3) or (%d,); got %s" % (self.blobs_per_body, 3 * self.blobs_per_body, sb.shape))
        if scale is not None:
            scale = np.asarray(scale, dtype=np.float64)
            if scale.shape != (self.N_bodies,):
                _fail("scale must have shape (%d,); got %s" % (self.N_bodies, scale.shape))
        self.ctx.set_body_slip(sb, scale, on=on)

    def flow_slip(self):
        """the flow model's term at every replica's configuration, (R, n3)"""
        return self.ctx.ensemble_flow_slip()

    def record_moments(self, on=True):
        """every step from now on leaves the first moments of its lambda on the device (one launch over R N_bod bodies)"""
        self.ctx.record_moments(on)

    def step_moments(self):
        """first moments D_b = sum (r_i - X_b) lambda_i^T recorded by the last step, (R, N_bod, 3, 3)"""
        return self.ctx.ensemble_step_moments()

    def close(self):
        self.ctx.close()
