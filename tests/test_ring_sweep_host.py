"""The ring sweep's table and references (tests/test_gpu_ring_descriptor_sweep.py), checked on the
CPU with the oracle alone: every entry is a shape the ring engines' gate admits (restated from
nrt_launch.h: whoever changes the gate must re-pick the table), between them they reach every nl
branch on both encoding widths, and the bar  max(1e-4 * scale, 4 * e32)  with its exact comparison
of hit / visible means what it reads: both outcomes are well populated, the MLP part is neither
negligible beside the spheres nor larger than an SDF's, the float32 oracle's own error leaves the
relative clause the governing one, few rays sit on the hit threshold, and no leaky_relu unit sits
on its kink where a normal is taken."""
import pytest

from tests.test_gpu_mlp_descriptor_sweep import nearest_kink
from tests.test_gpu_ring_descriptor_sweep import (CASES, EPS, FITTING, LDS, OVERSIZE, P, RAGGED,
                                                  REFRESH, bar, decided, gate, live_ksteps,
                                                  reference, scale_of, value_bar)

VALUES = ("origin", "scan", "occlusion")


def test_every_entry_passes_the_gate_and_the_oversize_one_fails_on_lds_only():
    for name in FITTING:
        ok, figures = gate(CASES[name])
        assert all(ok.values()), (name, ok, figures)
        # the split ring has no clause of its own in the gate: what ring32_supported admits fits
        assert figures["ring3"] + figures["tables"] <= LDS, (name, figures)
    for over_name, fit_name in OVERSIZE.items():
        ok, figures = gate(CASES[over_name])
        assert [k for k, v in ok.items() if not v] == ["lds"], (over_name, ok, figures)
        # ... by one sphere: the entry before it is the last count that fits
        fit, over = CASES[fit_name], CASES[over_name]
        assert over == fit._replace(spheres=fit.spheres + 1)
        assert all(gate(fit)[0].values())
    # one pair per clause of the LDS condition: the whole block's LDS at 256 wide, the 48 KiB of
    # tables at 128 wide
    f = {n: gate(CASES[n])[1] for n in OVERSIZE}
    assert f["lds_over"]["cap48"] and not f["lds_over"]["total"], f["lds_over"]
    assert f["lds48_over"]["total"] and not f["lds48_over"]["cap48"], f["lds48_over"]
    assert CASES["lds_over"].hidden == 256 and CASES["lds48_over"].hidden == 128


def test_every_nl_on_both_encoding_widths_and_the_rest_of_the_cover():
    nl = {48: set(), 80: set()}
    combos = set()
    for name in FITTING:
        c = CASES[name]
        ke = gate(c)[1]["ke"]
        n = live_ksteps(c.freqs) - (ke // 4 - 4)
        assert 1 <= n <= 4
        nl[ke].add(n)
        if n > 1:
            combos.add((c.hidden, c.activation))
    assert nl == {48: {1, 2, 3, 4}, 80: {1, 2, 3, 4}}, nl
    assert combos == {(h, a) for h in (128, 256) for a in ("softplus", "leaky_relu")}, combos
    cs = [CASES[n] for n in FITTING]
    assert {c.freqs for c in cs} >= {15, 16, 18, 20, 22, 31, 32, 34, 35, 38}
    assert {c.layers for c in cs} >= {1, 2, 3, 5, 8, 12, 18}
    assert {c.skip for c in cs if c.skip < c.layers} >= {1, 2, 3, 4}
    assert any(c.skip >= c.layers for c in cs)
    assert {c.spheres for c in cs} >= {0, 1, 3, 6, 13, 33, 100}
    assert any(c.out == 16 for c in cs)
    for name in list(RAGGED.values()) + list(REFRESH):
        c = CASES[name]
        assert live_ksteps(c.freqs) - (gate(c)[1]["ke"] // 4 - 4) > 1, name
    assert {gate(CASES[n])[1]["ke"] for n in REFRESH} == {48, 80}
    assert all(CASES[n].out == 1 for n in REFRESH)


@pytest.mark.parametrize("name", list(CASES))
def test_both_outcomes_are_populated(name):
    """At least 64 rays that hit at their origin and 64 that do not; the shadow rays likewise
    have both outcomes."""
    r = reference(name)
    hits = int((r["origin"][0] <= EPS).sum())
    assert 64 <= hits <= P - 64, hits
    vis = int((r["occlusion"][0] >= EPS).sum())
    assert 16 <= vis <= P - 16, vis


@pytest.mark.parametrize("name", list(CASES))
def test_the_mlp_part_is_visible_and_the_relative_clause_governs(name):
    """max|MLP part| in [0.05, 0.5] on every value tensor, and 4 * e32 <= 1e-4 * scale on every
    compared tensor: the bar is 1e-4 of the part the matrix cores compute, not something the
    reference's float32 noise has inflated."""
    r = reference(name)
    hit = r["origin"][0] <= EPS
    for key in VALUES:
        tol, e32, scale = value_bar(name, key)
        print(f"{name} {key}: scale {scale:.3g} e32 {e32:.3g} bar {tol:.3g}")
        assert 0.05 <= scale <= 0.5, (key, scale)
        assert 4 * e32 <= 1e-4 * scale, (key, e32, scale)
    # the march's t is compared on the rays that do not hit, the normals on those that do
    tol, e32, scale = value_bar(name, "origin", ~hit)
    assert 0.05 <= scale <= 0.5 and 4 * e32 <= 1e-4 * scale, (e32, scale)
    g64, g32, gy64 = (x[hit] for x in r["grad"])
    scale = scale_of(gy64)
    tol, e32 = bar(g64, g32, scale)
    print(f"{name} raw_n: scale {scale:.3g} e32 {e32:.3g} bar {tol:.3g}")
    assert 4 * e32 <= 1e-4 * scale, (e32, scale)


@pytest.mark.parametrize("name", list(CASES))
def test_few_rays_sit_on_the_threshold(name):
    """hit and visible are compared on every ray further than the value bar from eps; at most
    2 % of the rays are not."""
    for key in ("origin", "occlusion"):
        out = int((~decided(name, key)).sum())
        assert out <= 0.02 * P, (key, out)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.activation == "leaky_relu"])
def test_leaky_cases_take_no_normal_on_a_kink(name):
    """No float64 pre-activation within 1e-6 of zero at the origin of a ray that hits (the seeds
    of the table are picked for this): below that a float32 implementation may land on the other
    side and its gradient differ by the unit's whole weight."""
    r = reference(name)
    hit = r["origin"][0] <= EPS
    assert nearest_kink(r["ref"].mlp, r["rays"][hit][:, :3]) >= 1e-6
