"""GPU tier: the event cut-outs (fsea_extract_*, kernel fsea_extract_u8 in its three LDS sizes) over the argument domain a job
admits -- sample_offset + n_samples up to 2^52, |cycles_per_sample| up to 2^20, any finite phase0_cycles -- against the exact
reference, not against the zoom alone.

tests/test_gpu_extract.py holds a job's pairs to fsea.Zoom on the job's slice, bit for bit; the zoom is a second kernel built
from the same headers (fsea_fir_stage.h, fsea_zoom_image.h), so a fault in the shared arithmetic moves both.  Here every job
is held to tests/extract_ref.py's cutout_reference (tests/shift_ref.py: the phase in exact rational arithmetic, rounded once)
with MAX_ABS and MAX_REL of tests/test_gpu_fir.py as they stand.  Their derivation carries over for the reason the module
text of tests/test_gpu_shift_domain.py gives: the kernel's phase stays within 2^-30 cycles of exact over the whole domain
(tests/test_shift_ref_host.py), 1/32 of what the float conversion behind it adds; the taps are lowpass_like_taps (S = 1, DC
gain 1, the premises of those bounds).  MAX_ABS is asked of every output.  MAX_REL rests on rms(y) >= ~0.3 and on the
averaging of many outputs' errors, so it is asked of every job of at least ZOOM_TILE_OUTPUTS outputs and of all outputs of a
call together; the jobs of three to eight outputs (and the run-in of the long ones) have |y| far below 0.3 and are not held
to it singly (the docstring of test_fir_host_and_device_forms_against_the_exact_reference in tests/test_gpu_shift_domain.py).

The grid is tests/test_extract_host.py's domain_jobs, whose CPU tests say what it holds: the positions of grid_positions and
a job with 2^32 inside its second tile, every GRID_CYCLES x GRID_PHASES across 2^31 and at the last admissible job, and all
64 pairs (first mod 8, sample_offset mod 8) above 2^40 and below 8, where the first group's base lies in front of stream
position 0 -- the kernel's own staging (stage_group_at: groups aligned to the buffer, o, turned[]) that the zoom has no
counterpart of.  Three calls per case, the tables laid out in another order than the table's; beside the reference, bit
identity with the zoom (which says whose fault a failure is) and of the host form, guard bands, padding and input."""
import numpy as np
import pytest

from frequensea_amd import fsea
from tests import extract_ref as R
from tests.guarded import FILL, Guarded
from tests.test_extract_host import DOMAIN_CASES, domain_calls, domain_jobs
from tests.test_gpu_extract import bits, laid_out, zoom_pairs
from tests.test_gpu_fir import MAX_ABS, MAX_REL
from tests.test_gpu_zoom import lowpass_like_taps

pytestmark = pytest.mark.gpu

T = fsea.ZOOM_TILE_OUTPUTS


def rel_l2(got, want):
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30))


@pytest.mark.parametrize("D,L,flip", DOMAIN_CASES)
def test_every_job_of_the_domain_grid_against_the_exact_reference(D, L, flip):
    c = lowpass_like_taps(L, 100 * D + L)
    ex, zoom = fsea.Extract(c, D), fsea.Zoom(c, D, 128)
    groups, n_iq = domain_jobs(D, L)
    rng = np.random.default_rng(1000 * D + L + flip)
    iq = rng.integers(0, 256, 2 * n_iq, dtype=np.uint8)
    d_iq = Guarded(iq.nbytes).upload(iq)
    worst_abs = worst_rel = 0.0
    for k, jobs in enumerate(domain_calls(groups)):
        order = [int(i) for i in rng.permutation(len(jobs))]
        table, total = laid_out(ex, jobs, order)
        assert [j.out_first for j in table] != sorted(j.out_first for j in table)
        g_pairs = Guarded(8 * total)
        ex.run_device(d_iq.addr, n_iq, table, g_pairs.addr, total, flip=bool(flip))
        got = g_pairs.payload(np.complex64, (total,))
        g_pairs.check("D=%d L=%d call %d: a payload of exactly total_pairs pairs" % (D, L, k))
        d_iq.check("the input is read, not written")
        host = ex.run(iq, jobs, flip=bool(flip))
        owned = np.zeros(total, bool)
        failures, every_got, every_want = [], [], []
        for i, (j, mine) in enumerate(zip(table, host)):
            n_out = j.n_samples // D
            what = (i, j.first, j.n_samples, j.sample_offset, j.cycles_per_sample, j.phase0_cycles)
            pairs = got[j.out_first:j.out_first + n_out]
            assert not owned[j.out_first:j.out_first + n_out].any() and n_out == ex.out_pairs(j.n_samples) >= 3
            owned[j.out_first:j.out_first + n_out] = True
            want = R.cutout_reference(iq, j, c, D, flip)
            assert want.shape == pairs.shape
            err = float(np.abs(pairs.astype(np.complex128) - want).max())
            rel = rel_l2(pairs.astype(np.complex128), want) if n_out >= T else 0.0
            worst_abs, worst_rel = max(worst_abs, err), max(worst_rel, rel)
            as_zoom = np.array_equal(bits(pairs), bits(zoom_pairs(zoom, iq, j, flip)))
            as_host = np.array_equal(bits(pairs), bits(mine))
            if not (err <= MAX_ABS and rel <= MAX_REL and as_zoom and as_host):
                failures.append(what + ("max |delta| %.3e" % err, "rel L2 %.3e" % rel, "== zoom: %s" % as_zoom, "== host form: %s" % as_host))
            every_got.append(pairs.astype(np.complex128))
            every_want.append(want)
        rel = rel_l2(np.concatenate(every_got), np.concatenate(every_want))
        worst_rel = max(worst_rel, rel)
        print("D=%d L=%d flip=%d call %d: %d jobs, %d pairs, relative L2 of the call %.3e" % (D, L, flip, k, len(jobs), int(owned.sum()), rel))
        assert not failures, (D, L, flip, k, len(failures), failures[:8])
        assert rel <= MAX_REL, (D, L, flip, k, rel)
        raw = g_pairs.payload(np.uint8, (total, 8))
        assert 0 < (~owned).sum() and np.all(raw[~owned] == FILL)      # odd outputs leave padding pairs: still the fill
        g_pairs.free()
    assert np.array_equal(d_iq.payload(np.uint8, iq.shape), iq)
    print("D=%d L=%d flip=%d: worst max |delta| %.3e, worst relative L2 %.3e" % (D, L, flip, worst_abs, worst_rel))
    d_iq.free()
    ex.close()
    zoom.close()
