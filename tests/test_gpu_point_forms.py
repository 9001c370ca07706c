"""The group law of csrc/curve.hpp ON THE DEVICE (bpmi_debug_point_op) at every limb form its contract admits: limb for limb
against the host build of the same header (t_point_op), and decoded against the oracle's affine group law.  The cases are those
of tests/test_point_forms.py: every input coordinate in every non-canonical form, P + P, P + (-P), the identity on either side
and on both, mixed with general cases inside the same waves."""
import ctypes
import random

import pytest

from test_csrc_host import shim  # noqa: F401
from test_point_forms import NAMES, OPS, check_against_oracle, flat, host_point_op, point_cases

pytestmark = pytest.mark.gpu


def test_device_group_law_equals_host_limb_for_limb(shim):  # noqa: F811
    import gpu_common
    eng = gpu_common.engine()
    for op in sorted(OPS):
        cases = point_cases(op, random.Random(1000 + op), n_random=1500)
        n = len(cases)
        out = (ctypes.c_uint32 * (36 * n))()
        eng._ck(eng.lib.bpmi_debug_point_op(eng.ctx, op, flat([c[0] for c in cases]), flat([c[1] for c in cases]), n, out))
        got = list(out)
        dev = [got[36 * i: 36 * i + 36] for i in range(n)]
        host = host_point_op(shim, op, cases)
        for i in range(n):
            assert dev[i] == host[i], (NAMES[op], i, cases[i][0], cases[i][1])
        check_against_oracle(op, cases, dev)
