"""Bulk hash to the curve on the GPU (bpmi_ec_hash_batch / _range and their _dev forms, csrc/h2c_kernels.hpp) against the oracle's
elliptic_hash: the reference's own outputs, the 4 096 messages str(i) || b"gs" with the counters they stop at, the sizes and padding
edges at which the kernels take another path, max_tries, the refusals, and the derived generators as MSM input without a host hop.
A call of up to 196 608 messages runs the loop per lane (k_h2c_plain), so the per-wave queue (k_h2c_queue, the kernel of larger
calls) is driven through the option "h2c_per_lane": 1, 3 (a span that ends inside a row) and 64 (the whole set as ONE wave, 64 claims
per lane)."""
import pytest

import h2c_ref
import helpers
from h2c_ref import IDENTITY
from oracle import cbind

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import gpu_common
    return gpu_common.engine()


@pytest.fixture()
def option(eng):
    """set engine options for one test, and put the defaults back"""
    touched = []

    def set_option(name, value):
        touched.append(name)
        eng.set_option(name, value)
    yield set_option
    for name in touched:
        eng.set_option(name, 0)


def split(packed):
    return [packed[i: i + 64] for i in range(0, len(packed), 64)]


def test_reference_outputs(eng, golden):
    rows = golden("hash_codec.json")["elliptic_hash"]
    assert len(rows) == 10
    got = eng.ec_hash_batch_bytes([bytes.fromhex(m) for m, _ in rows])
    assert split(got) == [int(x, 16).to_bytes(32, "little") + int(y, 16).to_bytes(32, "little") for _, (x, y) in rows]


@pytest.mark.parametrize("plain,per_lane", [(0, 0), (0, 1), (0, 3), (0, 64), (1, 0)])
def test_range_form_full_set(eng, option, plain, per_lane):
    """points and counters equal the oracle's; the set holds the counters 10, 13, 10 and 11 (i = 1397, 1616, 2521, 3041): the counter's
    step from one digit to two happens inside a lane's loop"""
    want_pts, want_tries = h2c_ref.gs_set()
    assert {i: t for i, t in enumerate(want_tries) if t >= 10} == {1397: 10, 1616: 13, 2521: 10, 3041: 11}
    option("h2c_plain", plain)
    option("h2c_per_lane", per_lane)
    pts, tries = eng.ec_hash_range_bytes(b"gs", 0, 4096, with_tries=True)
    assert list(tries) == want_tries
    assert split(pts) == want_pts


def test_all_four_forms_agree(eng):
    want_pts, want_tries = h2c_ref.gs_set()
    want = b"".join(want_pts)
    msgs = [b"%dgs" % i for i in range(4096)]
    pts, tries = eng.ec_hash_batch_bytes(msgs, with_tries=True)
    assert pts == want and list(tries) == want_tries
    buf, tries = eng.ec_hash_batch_dev(msgs, with_tries=True)
    assert buf.download(64 * 4096) == want and list(tries) == want_tries
    buf2 = eng.alloc(64 * 4096)
    assert eng.ec_hash_range_dev(b"gs", 0, 4096, d_out=buf2) is buf2
    assert buf2.download() == want
    assert eng.ec_hash_range_bytes(b"gs", 0, 4096) == want


@pytest.mark.parametrize("per_lane", [0, 2])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_sizes(eng, option, n, per_lane):
    want_pts, want_tries = h2c_ref.gs_set()
    option("h2c_per_lane", per_lane)
    pts, tries = eng.ec_hash_range_bytes(b"gs", 0, n, with_tries=True)
    assert split(pts) == want_pts[:n] and list(tries) == want_tries[:n]
    pts, tries = eng.ec_hash_batch_bytes([b"%dgs" % i for i in range(n)], with_tries=True)
    assert split(pts) == want_pts[:n] and list(tries) == want_tries[:n]


def test_window_with_a_digit_count_change(eng):
    """lo != 0, and the index grows from six digits to seven inside the span"""
    want_pts, want_tries = h2c_ref.oracle_range(b"gs", 999990, 1000010)
    pts, tries = eng.ec_hash_range_bytes(b"gs", 999990, 1000010, with_tries=True)
    assert split(pts) == want_pts and list(tries) == want_tries
    lo = 2**32 - 3                                                         # the last indices there are
    want_pts, want_tries = h2c_ref.oracle_range(b"", lo, 2**32)
    pts, tries = eng.ec_hash_range_bytes(b"", lo, 2**32, with_tries=True)
    assert split(pts) == want_pts and list(tries) == want_tries


@pytest.mark.parametrize("tail_len", [53, 54, 55, 61, 62, 63, 117, 118, 119])
def test_padding_edges(eng, tail_len):
    """twelve messages per tail length: with one or two counter digits and one or two index digits in front, the total lengths
    straddle 55 / 56, 63 / 64 and 119 / 120, where either hash takes one more block"""
    tail = bytes((11 * k + tail_len) & 0xFF for k in range(tail_len))
    want_pts, want_tries = h2c_ref.oracle_range(tail, 0, 12)
    pts, tries = eng.ec_hash_range_bytes(tail, 0, 12, with_tries=True)
    assert split(pts) == want_pts and list(tries) == want_tries
    pts, tries = eng.ec_hash_batch_bytes([b"%d" % i + tail for i in range(12)], with_tries=True)
    assert split(pts) == want_pts and list(tries) == want_tries


def test_a_long_message_among_short_ones(eng):
    msgs = [b"a", b"", bytes(range(256)) * 19 + b"x" * 136, b"bc", b"gs"]
    assert len(msgs[2]) == 5000
    want = [h2c_ref.oracle_one(m) for m in msgs]
    pts, tries = eng.ec_hash_batch_bytes(msgs, with_tries=True)
    assert split(pts) == [p for p, _ in want] and list(tries) == [t for _, t in want]


@pytest.mark.parametrize("per_lane", [0, 4])
def test_max_tries(eng, option, per_lane):
    from bulletproofs_amd.engine import EngineError
    want_pts, want_tries = h2c_ref.gs_set()
    option("h2c_per_lane", per_lane)
    pts, tries = eng.ec_hash_range_bytes(b"gs", 0, 4096, max_tries=1, with_tries=True)
    assert list(tries) == [1 if t == 1 else 0 for t in want_tries]
    assert split(pts) == [p if t == 1 else IDENTITY for p, t in zip(want_pts, want_tries)]
    # without a tries array an identity must not pass for a generator: the call names the first message without a point.  (The
    # oracle stops at counter 1 for "0gs" and "1gs" and at 3 for "2gs": that index is 2.)
    first = next(i for i, t in enumerate(want_tries) if t != 1)
    assert first == 2
    with pytest.raises(EngineError, match=r"message %d has no point" % first):
        eng.ec_hash_range_bytes(b"gs", 0, 4096, max_tries=1)
    with pytest.raises(EngineError, match=r"message %d has no point" % first):
        eng.ec_hash_batch_dev([b"%dgs" % i for i in range(100)], max_tries=1)
    pts, tries = eng.ec_hash_range_bytes(b"gs", 0, 4096, max_tries=255, with_tries=True)
    assert 0 not in tries and split(pts) == want_pts
    assert eng.ec_hash_range_bytes(b"gs", 0, 4096, max_tries=13) == b"".join(want_pts)      # the largest counter of the set


def test_refusals(eng):
    from bulletproofs_amd.engine import EngineError
    good = h2c_ref.gs_set()[0][:3]
    for call in (lambda: eng.ec_hash_batch_bytes(b"abcdef", offsets=[0, 4, 2]),
                 lambda: eng.ec_hash_batch_bytes([b"ab", b"a" * 65536]),
                 lambda: eng.ec_hash_range_bytes(b"gs", 2**32 - 2, 2**32 + 1),
                 lambda: eng.ec_hash_range_bytes(b"gs", 5, 4),
                 lambda: eng.ec_hash_range_bytes(b"a" * 65536, 0, 2),
                 lambda: eng.ec_hash_range_bytes(b"gs", 0, 3, max_tries=256),
                 lambda: eng.ec_hash_batch_bytes([b"0gs"], max_tries=256),
                 lambda: eng.ec_hash_range_dev(b"gs", 0, 2**26 + 1)):
        with pytest.raises(EngineError, match="error -3"):
            call()
        assert split(eng.ec_hash_range_bytes(b"gs", 0, 3)) == good                    # a following good call succeeds
    assert eng.ec_hash_batch_bytes([b"a" * 65535]) == h2c_ref.oracle_one(b"a" * 65535)[0]     # the longest message there is


def test_derived_generators_are_msm_input(eng):
    """64 + 64 generators derived on the device and multiplied there: no host hop between the two"""
    from bulletproofs_amd.utils import elliptic_hash_range
    from bulletproofs_amd.engine import DeviceBuffer
    scalars = helpers.scal(64, helpers.seed(9))
    d_s = eng.upload(cbind.pack_scalars([int(s.x) if hasattr(s, "x") else int(s) for s in scalars]))
    for s in (helpers.seed(1), helpers.seed(2)):
        d_g = elliptic_hash_range(s, 0, 64, device=True, engine=eng)
        assert isinstance(d_g, DeviceBuffer) and d_g.nbytes == 64 * 64
        want = cbind.msm(helpers.gens(64, s), [int(v.x) if hasattr(v, "x") else int(v) for v in scalars])
        assert eng.msm_dev(d_g, d_s, 64) == cbind.pack_points([want])


def test_utils_surface(eng):
    from bulletproofs_amd.ec import PackedPoints
    from bulletproofs_amd.utils import elliptic_hash, elliptic_hash_batch, elliptic_hash_range
    want_pts, _ = h2c_ref.gs_set()
    pts = elliptic_hash_range(b"gs", 5, 70, engine=eng)
    assert isinstance(pts, PackedPoints) and pts.packed == b"".join(want_pts[5:70]) and len(pts) == 65
    one = elliptic_hash(b"7gs")
    assert (pts[2].x, pts[2].y) == (one.x, one.y)
    batch = elliptic_hash_batch([b"%dgs" % i for i in range(5, 70)], engine=eng)
    assert batch.packed == pts.packed
