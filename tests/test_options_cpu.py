"""The option table behind bpmi_set_option (python-bulletproofs_amd/csrc/options_host.hpp) checked on the CPU:
tests/csrc_host/options_main.cpp, a stand-alone program, is compiled with the host compiler (address and undefined-behaviour sanitizers
on), prints the table and runs option_set on every probe of tests/option_cases.py -- the list transcribed from the strcmp chain the table
replaced.  The same list pins the entry point itself in tests/test_gpu_abi_errors.py."""
import json
import os
import re
import subprocess

import pytest

from option_cases import CASES, UNKNOWN, probes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "csrc_host", "options_main.cpp")
INC = os.path.join(REPO, "python-bulletproofs_amd", "csrc")
E_ARG = -3
PROBES = probes()


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """(the rows, the result of every probe, the result of every unknown name): one build, one run."""
    exe = str(tmp_path_factory.mktemp("options") / "options_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe])
    args = [str(x) for p in PROBES for x in p[:2]] + [x for name in UNKNOWN for x in (name, "0")]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(lines) == 1 + len(PROBES) + len(UNKNOWN)
    return lines[0]["rows"], lines[1:1 + len(PROBES)], lines[1 + len(PROBES):]


def test_the_rows_and_their_defaults(table):
    rows = table[0]
    names = [r["name"] for r in rows]
    assert len(rows) == 62 and len(set(names)) == 62
    # tests restore an option by setting its default: the row must take it
    assert all(r["default_ok"] == 1 for r in rows), [r["name"] for r in rows if not r["default_ok"]]
    assert sorted(r["name"] for r in rows if r["wide"]) == ["ipa_big_m", "ipa_small_m"]
    # the case list covers the table, name by name, and knows the same defaults
    assert sorted(names) == sorted(c[0] for c in CASES) and len(CASES) == 62
    assert {r["name"]: r["default"] for r in rows} == {c[0]: c[1] for c in CASES}


def test_every_option_is_documented_in_the_header(table):
    text = open(os.path.join(REPO, "include", "bpmi.h")).read()
    comment = re.search(r"/\* tuning knobs.*?\*/\s*int bpmi_set_option\(", text, re.S)
    assert comment, "the option comment above bpmi_set_option"
    missing = [r["name"] for r in table[0] if '"%s"' % r["name"] not in comment.group(0)]
    assert not missing, missing


def test_accepted_values_messages_and_effects(table):
    _, results, _ = table
    for (name, value, ok, msg, effect), got in zip(PROBES, results):
        tag = (name, value, got)
        assert got["rest_same"] == 1, tag
        if ok:
            assert (got["rc"], got["msg"], got["fx"]) == (0, "", effect), tag
            # stored as it is; an int member keeps the low 32 bits of a wider value (only "rp_rows" takes one)
            want = value if name in ("ipa_big_m", "ipa_small_m") else (value + (1 << 31)) % (1 << 32) - (1 << 31)
            assert got["stored"] == want, tag
            assert want == value or name == "rp_rows", tag
        else:
            assert (got["rc"], got["msg"], got["fx"]) == (E_ARG, msg, "none"), tag


def test_an_unknown_name_is_refused(table):
    for name, got in zip(UNKNOWN, table[2]):
        assert (got["rc"], got["msg"], got["fx"], got["rest_same"]) == (E_ARG, "unknown option " + name, "none", 1), name
