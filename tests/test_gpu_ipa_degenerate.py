"""The inner-product prover's generator folds on COLLIDING generators, against integers.

Every generator is a known multiple of G (tests/ipa_dlog_ref.py), so every L and R, every exported generator and the final scalars
are Python integers times G: equal, opposite and identity generators, challenges 1, -1, iota, lambda, x then 1/x.  That drives the
fold kernels through what uniformly random inputs never reach -- acc == addend and acc == -addend inside the ladders, identities
written by one kernel and read by the next, whole waves of identity outputs, GLV halves 0 and +-1 -- on every route bpmi_ipa_fold
can take (the predicates of csrc/ipa_host.hpp), at the smallest length that reaches each.  test_ipa_dlog_ref_cpu.py proves that
each scenario shows its edge; here everything the engine returns must equal the model's bytes exactly."""
import functools

import pytest

import ipa_dlog_ref as D
from ipa_dlog_ref import Q

pytestmark = pytest.mark.gpu

DEFAULTS = {"ipa_big_m": 0, "ipa_small_m": 0, "fold_wnaf": 2, "fold_shared": 1, "ipa_small_step": 0, "mul_batch_glv": 1}
ALL = tuple(D.SCENARIOS)
# path -> (n, options, scaled forms, scenarios, (generator-fold launches, batched multiplications) of one proof)
PATHS = {
    # M = 1024 >= big_m, four deferred folds, then 1024 -> 64: k_ec_odd_multiples<16> + the ladder chosen by fold_wnaf (64 % 64 == 0: GLV)
    "ladder_glv": (1024, {"ipa_big_m": 256, "ipa_small_m": 1}, (False,), ALL, (1, 0)),
    "ladder_w4": (1024, {"ipa_big_m": 256, "ipa_small_m": 1, "fold_wnaf": 1}, (False,), ALL, (1, 0)),
    "ladder_naf": (1024, {"ipa_big_m": 256, "ipa_small_m": 1, "fold_wnaf": 0}, (False,), ALL, (1, 0)),
    # 4096 -> 256 -> 16: the second fold builds its tables from the first one's outputs (256 points) and folds to 16 (k_ec_multifold_w4)
    "two_ladders": (4096, {"ipa_big_m": 64, "ipa_small_m": 1}, (False,), ALL, (2, 0)),
    # 1024 < big_m, product fold at length 64, K = 16: k_ec_fold_glv + k_ec_sum_partials
    "products_shared": (1024, {"ipa_small_m": 64}, (False,), ALL, (1, 0)),
    # ... k_ipa_fold_scalars + bit-serial k_ec_mul_batch (2 M = 2048) + k_ec_sum_strided
    "products_per_lane": (1024, {"ipa_small_m": 64, "fold_shared": 0}, (False,), ALL, (1, 1)),
    # ... 2 M = 32 768: k_ec_odd_multiples<4> + k_ec_mul_batch_glv
    "products_per_lane_glv": (16384, {"ipa_small_m": 1024, "fold_shared": 0}, (False,),
                              ("control", "all_equal_ones", "halves_equal_iota", "identities"), (1, 1)),
    # a per-generator scale sends the product fold per lane whatever fold_shared says: the hscale branch of k_ipa_fold_scalars / k_ipa_expand
    "products_scaled": (1024, {"ipa_small_m": 64}, (True,), ALL, (1, 1)),
    # fold of a, b, the coefficient tables and the next round's preparation in one launch, plain and scaled
    "one_launch_step": (512, {"ipa_small_step": 1}, (False, True), ALL, (0, 0)),
    # never folded: k_ipa_coef_update, k_ipa_expand to 64 coefficients, k_ipa_export_scalars at every length
    "deferred_only": (64, {}, (False, True), ALL, (0, 0)),
}


@pytest.fixture(scope="module")
def gp():
    import gpu_common
    return gpu_common


@functools.lru_cache(maxsize=None)
def expected(name, n, scaled):
    """The model's trace and the case's wire bytes, computed once and shared by the paths of the same length."""
    events, (sg, sh, su, a, b, xs, hscale) = D.expected_trace(name, n, scaled)
    pts = D.dlogs_to_le64(sg + sh + [su])          # at most 4 POOL + 1 multiplications of G, whatever n is
    wire = (b"".join(pts[:n]), b"".join(pts[n:2 * n]), D.pack_scalars(a), D.pack_scalars(b), pts[2 * n],
            None if hscale is None else D.pack_scalars(hscale))
    return events, wire, xs


def run_case(eng, name, n, scaled):
    """The engine through the raw state object, compared event by event; -> None or the first difference."""
    events, (gb, hb, ab, bb, ub, hs), xs = expected(name, n, scaled)
    st = eng.ipa_create(gb, hb, ab, bb, n, ub, hs)
    try:
        r = 0
        for ev in events:
            if ev[0] != "finish" and ev[1] < len(st):
                st.fold(xs[r], pow(xs[r], -1, Q))
                r += 1
            where = "scenario %s%s, length %d (after %d folds): %s" % (name, " scaled" if scaled else "", len(st), r, ev[0])
            if ev[0] == "LR":
                assert len(st) == ev[1], where
                L, R = st.round_LR()
                if L != ev[2]:
                    return where + " L"
                if R != ev[3]:
                    return where + " R"
            elif ev[0] == "export":
                assert len(st) == ev[1], where
                for what, g, w in zip(("g", "h", "a", "b"), st.export(), ev[2:]):
                    if g != w:
                        size = 64 if what in "gh" else 32
                        bad = [i for i in range(ev[1]) if g[size * i: size * i + size] != w[size * i: size * i + size]]
                        return where + " %s at %s" % (what, bad[:8])
            elif st.finish() != ev[1:]:
                return where
    finally:
        st.close()
    return None


@pytest.mark.parametrize("path", list(PATHS))
def test_ipa_degenerate_generators_vs_integers(gp, path):
    n, options, scaled_forms, names, _ = PATHS[path]
    eng = gp.engine()
    failures = []
    try:
        for k, v in dict(DEFAULTS, **options).items():
            eng.set_option(k, v)
        for name in names:
            for scaled in scaled_forms:
                bad = run_case(eng, name, n, scaled)
                if bad:
                    failures.append(bad)
    finally:
        for k, v in DEFAULTS.items():
            eng.set_option(k, v)
    assert not failures, "path %s: %d of %d cases differ from the integer model:\n  " % (
        path, len(failures), len(names) * len(scaled_forms)) + "\n  ".join(failures)



@pytest.mark.parametrize("path", list(PATHS))
def test_every_path_reaches_its_generator_fold(gp, path):
    """The options above are read from the predicates of ipa_host.hpp; if those move, a path could stop reaching its kernels and
    still pass.  Stage counters of one control proof: the generator folds ("ec_lincomb2": one timed launch group per fold) and the
    batched multiplication of the per-lane product fold ("ec_mul_batch") run exactly as often as the path says -- and the values
    are the model's with the event timers on, too."""
    n, options, scaled_forms, _, (folds, muls) = PATHS[path]
    eng = gp.engine()
    try:
        for k, v in dict(DEFAULTS, **options).items():
            eng.set_option(k, v)
        eng.profile(True)
        eng.profile_reset()
        bad = run_case(eng, "control", n, scaled_forms[-1])
        prof = eng.profile_read()
    finally:
        eng.profile(False)
        for k, v in DEFAULTS.items():
            eng.set_option(k, v)
    assert bad is None, bad
    assert (prof["ec_lincomb2"][1], prof["ec_mul_batch"][1]) == (folds, muls), path
