"""The configurations that tests/test_periodic_cpu.py and tests/test_periodic_gpu.py share, so that the CPU test checks the
positivity of M_per exactly where the GPU tests take roots and Brownian steps.  Plain numpy."""
import numpy as np


def blob_positions(cfg, X, Q):
    """r_k = X_b + R(Q_b) c_k, body-major (N_bod N_blb, 3); cfg with its mean removed, Q normalised"""
    from oracle import oracle as O
    cfg = O.remove_mean(cfg)
    Qn = O.normalize_quats(Q)
    return np.concatenate([cfg @ O.rot_matrix(Qn[b]).T + np.asarray(X, dtype=np.float64).reshape(-1, 3)[b] for b in range(Qn.shape[0])])


def spacing(a):
    return 2.0 * (1.0 + a) + 0.5                              # make_config's lattice


def layer10():
    """10 x shell_N_12 of make_config(10, 12, wall): a 3 x 3 x 2 lattice (one body in the upper layer), in a cell of three
    lattice spacings by three plus 0.7: the bodies of the first and the last column / row are neighbours across both boundaries"""
    from rigid_body_light_amd.synth import make_config
    c = make_config(10, 12, True)
    s = spacing(c["a"])
    c["L"] = (3.0 * s, 3.0 * s + 0.7)
    c["r"] = blob_positions(c["cfg"], c["X"], c["Q"])
    return c
