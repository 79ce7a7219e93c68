"""Ensembles of independent replicas of one small system (include/rbl.h section 5).

    ens = Ensemble(cfg, X, Q, a, eta, dt, kBT=1.0, wall=True)     # X (R, N_bod, 3), Q (R, N_bod, 4)
    ens.set_interactions(w=0.5, eps_wall=4.0, b_wall=0.1)
    for n in range(steps):
        ens.step_brownian(np.zeros(6), seed=n)                    # every replica, a fixed number of launches
    X, Q = ens.get_config()

All replicas share the structure, the parameters, the wall flag and the force model; each has its own configuration, resident on
the GPU.  Replicas never interact.  Sizes are those of the one-kernel solver (N_bod N_blb <= 256, N_bod <= 64) and 1 <= R <= 65535.
"""
import numpy as np

from ._lib import DeviceContext


def _fail(message):
    raise ValueError(message)


class Ensemble:
    def __init__(self, rigid_config, X, Q, a, eta, dt, kBT=1.0, wall=False):
        template = np.asarray(rigid_config, dtype=np.float64)
        if template.size % 3:
            _fail("rigid_config must have length 3 N_blb; got shape %s" % (template.shape,))
        self.blobs_per_body = template.size // 3
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

    def step_deterministic(self, F, max_iter=50, rtol=1e-8):
        """one deterministic step of every replica -> (iterations (R,), residual estimates (R,))"""
        return self.ctx.ensemble_step_deterministic(self._forces(F), max_iter=max_iter, rtol=rtol)

    def step_brownian(self, F, W=None, seed=0, split_rand=True, delta=1e-4, max_iter=50, rtol=1e-8):
        """one stochastic midpoint step of every replica -> (iterations (R,), residual estimates (R,)).  W: (R, 9 N_bod N_blb)
        standard normals [W1 | W2 | W_rfd] per replica, or None to draw them from `seed` (replica r from its own counters)"""
        F = self._forces(F)
        if W is not None:
            W = np.asarray(W, dtype=np.float64)
            n = 9 * self.N_bodies * self.blobs_per_body
            if W.shape != (self.R, n):
                _fail("W must have shape (%d, %d); got %s" % (self.R, n, W.shape))
        return self.ctx.ensemble_step_brownian(F, W=W, seed=seed, split_rand=split_rand, delta=delta, max_iter=max_iter, rtol=rtol)

    def set_interactions(self, w=0.0, eps_wall=0.0, b_wall=1.0, eps_blob=0.0, b_blob=1.0, r_cut=None, on=True):
        """the force model of RigidBody.set_interactions, for every replica (steric pairs only inside a replica)"""
        self.ctx.set_interactions(w=w, eps_wall=eps_wall, b_wall=b_wall, eps_blob=eps_blob, b_blob=b_blob, r_cut=r_cut, on=on)

    def interaction_forces(self):
        """body forces and torques of the model, (R, 6 N_bod), reference convention (-K^T f_phys)"""
        return self.ctx.ensemble_interaction_forces()[0]

    def interaction_energy(self):
        """total potential energy of every replica, (R,)"""
        return self.ctx.ensemble_interaction_forces()[1]

    def close(self):
        self.ctx.close()
