#!/usr/bin/env python3
"""The flow around a roller: one shell of 162 blobs above a wall, driven by a torque about y and pulled down by its weight.
One saddle solve gives the blob forces lambda and the body velocity U; RigidBody.velocity_field then evaluates the fluid
velocity on an x-z plane through the body (include/rbl.h section 6).  Saves flow_field.npz (x, z, u on the grid) and prints
one JSON line: the largest speed on the grid, the largest speed in the grid row nearest the wall (z = 0.01 a), and the
relative residual of u at the blobs against K U (the no-slip condition the solve imposed).  No plotting dependency:
    python examples/flow_field.py [--nx 128] [--nz 64] [--out flow_field.npz]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from rigid_body_light_amd import RigidBody, load_structure


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=128)
    ap.add_argument("--nz", type=int, default=64)
    ap.add_argument("--out", default="flow_field.npz")
    args = ap.parse_args()
    params, cfg = load_structure(162)
    a, eta = params["sep"] / 2.0, 1.0
    R = float(np.linalg.norm(cfg - cfg.mean(axis=0), axis=1).max()) + a     # the shell's outer radius
    X = np.array([[0.0, 0.0, R + 0.5 * a]])                                 # half a blob radius of gap under it
    Q = np.array([[1.0, 0.0, 0.0, 0.0]])
    rb = RigidBody(cfg, X, Q, a, eta, dt=0.01, wall_PC=True)
    n3 = 3 * rb.total_blobs
    F = np.array([0.0, 0.0, -1.0, 0.0, 2.0 * R, 0.0])                       # weight, torque about y
    rhs = np.concatenate([np.zeros(n3), -F])
    x, its, res = rb.solve_saddle(rhs, max_iter=200, rtol=1e-10)
    lam, U = x[:n3], x[n3:]
    # the x-z plane y = 0 through the body centre, first row just above the wall
    xs = np.linspace(-4.0 * R, 4.0 * R, args.nx)
    zs = 0.01 * a + np.linspace(0.0, 4.0 * R, args.nz)
    gz, gx = np.meshgrid(zs, xs, indexing="ij")
    pts = np.stack([gx.ravel(), np.zeros(gx.size), gz.ravel()], axis=1)
    u = rb.velocity_field(pts, lam)                                         # (nz nx, 3)
    speed = np.linalg.norm(u, axis=1).reshape(args.nz, args.nx)
    KU = rb.K_dot(U).reshape(-1)
    ub = rb.velocity_field(rb.get_blob_positions().reshape(-1), lam)        # u at the blobs: the no-slip velocity K U
    np.savez(args.out, x=xs, z=zs, u=u.reshape(args.nz, args.nx, 3), U=U, a=a)
    print(json.dumps({"grid": [args.nz, args.nx], "gmres_iters": int(its), "U": [float(v) for v in U],
                      "max_speed": float(speed.max()), "wall_row_z": float(zs[0]), "wall_row_max_speed": float(speed[0].max()),
                      "blob_residual": float(np.linalg.norm(ub - KU) / np.linalg.norm(KU)), "out": args.out}))


if __name__ == "__main__":
    main()
