#!/usr/bin/env python3
"""python tools/bench_velocity_field.py [--reps 10] -- rbl_velocity_field_dev (include/rbl.h section 6): cfg 3 sources x a 256 x 256 plane, cfg 2 x 64 x 64, 64 points x cfg 3 (the split path); one JSON line per case with ms, ps per pair, VALU per pair from the kernel's gfx950 assembly, the fp64 VALU issue fraction and k_apply_M<true>'s time per ordered pair on the same box.

Timing: device-resident inputs, hipEvents around `reps` back-to-back calls (pack + sweep + slab reduction), after one
warm-up call.  VALU per pair: the far sweep's inner loop of the k_vf_sweep instantiation the case launches (the blocks that
carry the pair arithmetic, no coincident-point branch), from `hipcc -S` of rbl_field.hip with the build's flags.  Issue
fraction = (pairs / 64 lanes) x VALU/pair x 4 cycles / (4 SIMDs x CUs x clock x time), at the sustained fp64 clock (SUSTAINED_GHZ) and
at the 2.4 GHz spec clock."""
import argparse, json, os, re, subprocess, sys, tempfile
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

SUSTAINED_GHZ = 2.05     # the clock the chip holds under fp64 VALU load
SPEC_GHZ = 2.4


def far_loop_valu(asm_lines, kernel_key, wall, ni):
    """VALU per pair of the far-sweep inner loop of one k_vf_sweep instantiation: of the innermost loops whose blocks hold
    exactly the NI pairs' v_rsq_f64 (2 per pair with the wall), the one with the fewest VALU in those blocks"""
    h = next(i for i, l in enumerate(asm_lines) if re.match(r"^_Z\S*" + kernel_key + r"\S*:", l))
    end = next(i for i in range(h, len(asm_lines)) if asm_lines[i].startswith(".Lfunc_end"))
    loops, cur = {}, None
    for l in asm_lines[h + 1:end]:
        m = re.match(r"^(?:\.LBB|; %bb\.)(\d+_\d+|\d+):(.*)$", l)
        if m:
            hm = re.search(r"Header=BB(\d+_\d+) Depth=2", m.group(2))
            label = m.group(1)
            cur = loops.setdefault(hm.group(1), []) if hm else None
            if cur is not None:
                cur.append([0, 0])
            continue
        if "This Inner Loop Header: Depth=2" in l:
            cur = loops.setdefault(label, [])
            cur.append([0, 0])
            continue
        t = l.strip().split(" ")[0].split("\t")[0] if l.strip() else ""
        if cur is None or not t or t.startswith((";", ".")):
            continue
        cur[-1][0] += t.startswith("v_")
        cur[-1][1] += t.startswith("v_rsq")
    best = None
    for blocks in loops.values():
        hot = [b for b in blocks if b[1] > 0]
        if sum(b[1] for b in hot) == (2 if wall else 1) * ni:
            v = sum(b[0] for b in hot) / ni
            best = v if best is None else min(best, v)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", default="plane256_cfg3,plane64_cfg2,points64_cfg3")
    args = ap.parse_args()
    from rigid_body_light_amd import make_config
    from rigid_body_light_amd._lib import DeviceContext
    from rigid_body_light_amd.build import HIPCC, ARCH, CSRC
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "rbl_field.s")
        subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=" + ARCH, "-x", "hip", "--offload-device-only", "-S",
                               "-Wno-unused-command-line-argument"] + os.environ.get("RBL_EXTRA_FLAGS", "").split()
                              + [os.path.join(CSRC, "rbl_field.hip"), "-o", asm])
        asm_lines = open(asm).read().split("\n")
    dev = torch.device("cuda:0")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    st = torch.cuda.current_stream()
    cases = {"plane256_cfg3": (200, 642, 256, 256), "plane64_cfg2": (50, 162, 64, 64), "points64_cfg3": (200, 642, 8, 8)}
    yard = {}
    for name in args.cases.split(","):
        nb, nblb, nx, nz = cases[name]
        wall = True
        c = make_config(nb, nblb, wall)
        ctx = DeviceContext(c["a"], c["eta"], wall, cfg=c["cfg"], dt=c["dt"], stream_ptr=st.cuda_stream)
        ctx.set_config(c["X"], c["Q"])
        N = nb * nblb
        d_r = torch.empty(3 * N, dtype=torch.float64, device=dev)
        ctx.multi_body_pos(d_r.data_ptr())
        r = d_r.cpu().numpy().reshape(-1, 3)
        lo, hi = r.min(axis=0), r.max(axis=0)
        # the x-z plane through the middle of the cluster, from just above the wall to above the top layer
        xs = np.linspace(lo[0] - 2.0, hi[0] + 2.0, nx)
        zs = np.linspace(0.01 * c["a"], hi[2] + 2.0, nz)
        gz, gx = np.meshgrid(zs, xs, indexing="ij")
        pts = np.stack([gx.ravel(), np.full(gx.size, 0.5 * (lo[1] + hi[1])), gz.ravel()], axis=1)
        P = pts.shape[0]
        d_p = torch.from_numpy(pts.reshape(-1)).to(dev)
        d_l = torch.from_numpy(np.random.default_rng(1).standard_normal(3 * N)).to(dev)
        d_u = torch.empty(3 * P, dtype=torch.float64, device=dev)
        ni, ch, wb = ctx.velocity_field_info(P, N)
        ctx.velocity_field_dev(d_p.data_ptr(), P, d_l.data_ptr(), d_r.data_ptr(), N, d_u.data_ptr())
        ctx.sync_check()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(args.reps):
            ctx.velocity_field_dev(d_p.data_ptr(), P, d_l.data_ptr(), d_r.data_ptr(), N, d_u.data_ptr())
        e1.record(st)
        ctx.sync_check()
        ms = e0.elapsed_time(e1) / args.reps
        # the yardstick: k_apply_M<true> (ordered pairs, the full row range) on these sources, same box
        if N not in yard:
            ctx.set_option("matvec_kernel", 1)
            d_o = torch.empty(3 * N, dtype=torch.float64, device=dev)
            ctx.apply_M(d_l.data_ptr(), d_r.data_ptr(), N, 0, N, d_o.data_ptr())
            ctx.sync_check()
            reps = max(2, args.reps // 2)
            e0.record(st)
            for _ in range(reps):
                ctx.apply_M(d_l.data_ptr(), d_r.data_ptr(), N, 0, N, d_o.data_ptr())
            e1.record(st)
            ctx.sync_check()
            yard[N] = e0.elapsed_time(e1) / reps * 1e9 / (float(N) * N)
            ctx.set_option("matvec_kernel", 0)
        ctx.close()
        pairs = float(P) * N
        valu = far_loop_valu(asm_lines, "k_vf_sweepILb%dELi%dE" % (1 if wall else 0, ni), wall, ni)
        issue = lambda ghz: (pairs / 64.0) * valu * 4.0 / (4.0 * n_cu * ghz * 1e9 * ms * 1e-3) if valu else None   # wave instructions
        print(json.dumps({"case": name, "points": P, "sources": N, "wall": wall, "ni": ni, "chunks": ch, "workspace_bytes": wb,
                          "ms": round(ms, 4), "ps_per_pair": round(ms * 1e9 / pairs, 4),
                          "kernel": "k_vf_sweep<%s,%d>" % ("true" if wall else "false", ni), "valu_per_pair": valu,
                          "valu_issue_frac_sustained": round(issue(SUSTAINED_GHZ), 4) if valu else None,
                          "valu_issue_frac_spec": round(issue(SPEC_GHZ), 4) if valu else None, "sustained_ghz": SUSTAINED_GHZ,
                          "k_apply_M_true_ps_per_ordered_pair": round(yard[N], 4)}), flush=True)


if __name__ == "__main__":
    main()
