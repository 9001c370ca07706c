#!/usr/bin/env python3
"""tests/golden/ipa_wire.json: the BPIP2 encodings (innerproduct/codec.py) of the REFERENCE-MADE Protocol-2 proofs of ipa.json at
n = 1 and n = 8 -- the plain proof and the one inside proof1 -- as hex.  The reference has no serialisation: these vectors pin OUR
byte layout on the reference's own proofs, so that a change of the codec, of the host encoder or of an expander cannot go unnoticed.
Needs no reference and no GPU (the inputs are the committed goldens):    python tests/golden/make_ipa_wire_golden.py"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import bulletproofs_amd  # noqa: E402,F401
from bulletproofs_amd.innerproduct.codec import proof2_to_bytes  # noqa: E402
import ipa_wire_common as W  # noqa: E402

if __name__ == "__main__":
    out = {}
    for case in W.golden_cases():
        if case["n"] in (1, 8):
            for name, w2 in W.golden_proofs(case):
                out["n%d.%s" % (case["n"], name)] = proof2_to_bytes(W.proof2_of(w2)).hex()
    with open(os.path.join(HERE, "ipa_wire.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote ipa_wire.json: %d encodings" % len(out))
