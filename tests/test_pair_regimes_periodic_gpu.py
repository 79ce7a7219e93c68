"""The periodic product kernel, one pair at a time: the sibling of tests/test_pair_regimes_gpu.py for k_apply_M_per<PX, PY>.

The same stars (tests/pair_probe.py: every height, position of the source's tile, radius and placement; wall only -- the cell is
not offered in free space), in a cell of 37.3 a x 41.9 a, commensurate with nothing in the star: the targets at r^ = 30 and 1000
fold onto near separations, so the kernel's nearest-image reduction, its image loop and its self / own image / other decision are
met by every pair class, where the sums of tests/test_periodic_gpu.py do not see one class that is wrong.  The periodic kernel calls
rbl_pair_accum in a form no other kernel uses: the folded displacement goes in as the row blob and the origin as the column blob.

Once per instantiation -- x and y with images (1, 1), x only (1, 0), y only (0, 1) -- at j-split 0 and 3.  The reference block of
target i against the source is periodic_oracle.block (120 targets x 9 images per star), damped like the sibling's reference.

    error = max |got - ref| / max(|block|_F, B_i B_j nf min(4/3, 1 / r^0)),   r^0 the NEAREST-IMAGE separation over a
    bound = pair_probe.bound(r^0, X) = 5e-13 + 6 eps (X / a) / r^0

The bound is the sibling's: the fold is one multiply, one rint and one fma on a difference that already carries eps X / a, and each
image adds one fma, relative to a separation no smaller than r^0.  No pair is skipped."""
import numpy as np
import pytest

import pair_probe as pp
import periodic_oracle as po

pytestmark = pytest.mark.gpu
ETA = 0.9
CELL = (37.3, 41.9)                                                   # in radii
INST = (("xy", (1.0, 1.0), (1, 1)), ("x", (1.0, 0.0), (1, 0)), ("y", (0.0, 1.0), (0, 1)))
PLACE = {0.0: "origin", 100.0: "100a", 1000.0: "1000a"}


def _reference(orc, st, L, n):
    """blocks[k] = B_i M_per[i, src] B_src for the source and every target i, and B_i B_src nf: the rows, their blocks, the units"""
    r, s, a = st["r"], st["src"], st["a"]
    rows = np.flatnonzero(st["target"] | (np.arange(len(r)) == s))
    B = orc.damp(r.reshape(-1), a).reshape(-1, 3)[:, 0]
    ref = np.empty((len(rows), 3, 3))
    for k, i in enumerate(rows):
        blk = po.block(orc, r[i], r[s], i, s, a, ETA, L, n) if i <= s else po.block(orc, r[s], r[i], s, i, a, ETA, L, n).T
        ref[k] = B[i] * B[s] * blk
    return rows, ref, B[rows] * B[s] / (8.0 * np.pi * ETA * a)


@pytest.mark.parametrize("off", pp.PLACEMENTS)
@pytest.mark.parametrize("a", pp.RADII)
def test_the_periodic_kernel_pair_by_pair(orc, a, off):
    """Measured on an MI355X, worst over heights, separations and directions, the three instantiations and both j-splits equal to
    two digits and equal to the open kernels' figures: 3.0e-14 at the origin, 4.3e-13 at 100 a, 2.6e-12 at 1000 a (bound there
    1.4e-11); r^0 >= 0.5 only: 3.0e-14 / 4.5e-14 / 4.1e-13; a = 1: <= 5.8e-15.  DESIGN.md 5a (last column) and 5c.  Under nx and ny
    swapped in PerCell every case fails (4.6e-4 of the scale in the x-only instantiation); with the ragged tile padded instead of
    cut short the cases with the source at the origin do (the source at height a sits on the padded slot: an overlap error)."""
    import torch
    from rigid_body_light_amd._lib import DeviceContext
    dev = torch.device("cuda:0")
    ctx = DeviceContext(a, ETA, True, stream_ptr=torch.cuda.current_stream().cuda_stream)
    ctx.set_option("matvec_kernel", 1)
    worst, failed = {}, []
    for hi, h in enumerate(pp.HEIGHTS):
        for w, where in enumerate(pp.WHERE):
            st = pp.star(a, h, off, where, (w + hi) % 3 - 1)
            N, s = len(st["r"]), st["src"]
            r = torch.from_numpy(st["r"].reshape(-1)).to(dev)
            F = torch.zeros(3, 3 * N, dtype=torch.float64, device=dev)
            for c in range(3):
                F[c, 3 * s + c] = 1.0
            out = torch.empty_like(F)
            _, X = pp.pair_geometry(st)
            for inst, on, n in INST:
                L = (CELL[0] * a * on[0], CELL[1] * a * on[1])
                rows, ref, unit = _reference(orc, st, L, n)
                d = st["r"][rows] - st["r"][s]
                rhat0 = np.linalg.norm(po.nearest(d, L), axis=1) / a
                assert po._folds(d, L).any()                          # a target whose nearest image is not the direct displacement
                lim = pp.bound(rhat0, X[rows])
                ctx.set_periodic(L[0], L[1], images=n)
                for js in (0, 3):
                    ctx.set_option("ordered_jsplit", js)
                    out.fill_(7.25)
                    for c in range(3):
                        ctx.apply_M(F[c].data_ptr(), r.data_ptr(), N, 0, N, out[c].data_ptr())
                    ctx.sync_check()                                  # no error flag
                    got = np.ascontiguousarray(out.cpu().numpy().reshape(3, N, 3).transpose(1, 2, 0))[rows]
                    err = pp.pair_errors(got, ref, rhat0, unit)
                    worst[inst] = max(worst.get(inst, 0.0), float(err.max()))
                    ok = rhat0 >= 0.5
                    worst[inst + ", r^0 >= 0.5 only"] = max(worst.get(inst + ", r^0 >= 0.5 only", 0.0), float(err[ok].max()))
                    if not (err <= lim).all():
                        k = int(np.argmax(err / lim))
                        failed.append("k_apply_M_per<%s> j-split %d, a=%.8g h_s/a=%g where=%s offset=%g: blob %d (%s, nominal r^ %g, tile %s) "
                                      "h_i/a=%.4g r^0=%.17g direct r^=%.6g: err %.3e bound %.3e"
                                      % (inst, js, a, h, where, off, rows[k], st["dirclass"][rows[k]], st["nominal"][rows[k]], st["tile"][rows[k]],
                                         st["r"][rows[k], 2] / a, rhat0[k], np.linalg.norm(d[k]) / a, err[k], lim[k]))
            ctx.set_option("ordered_jsplit", 0)
    ctx.close()
    for inst, v in sorted(worst.items()):
        print("PAIR-REGIMES-PERIODIC a=%-10.8g %-22s %-7s worst %.2e" % (a, inst, PLACE[off], v))
    assert not failed, "\n".join(failed)
