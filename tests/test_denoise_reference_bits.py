"""The bits of the CPU restatements (ptlumi.denoise.atrous_reference,
atrous_guided_reference, moments_reference) are pinned: SHA-256 digests of
their outputs on the GPU tests' own seeded inputs, recorded in
tests/golden/denoise_reference_bits.json before the restatements were folded
into one tap loop.  The GPU tests compare the kernels with the restatements;
this keeps the two from drifting together.  No GPU work here.

`python tests/test_denoise_reference_bits.py --write` records the digests of
the restatements as they stand (only for a deliberate change of a definition).
"""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PINNED = os.path.join(HERE, "golden", "denoise_reference_bits.json")

if __name__ == "__main__":
    sys.path.insert(0, HERE)
    import conftest  # noqa: F401  (registers the package as `ptlumi`)

from denoise_inputs import ITERATIONS, SIZES, case_key, reference_digest  # noqa: E402

CASES = [(name, w, h, it) for name in ("atrous", "atrous_guided") for (w, h) in SIZES for it in ITERATIONS]
CASES.append(("moments", None, None, None))


@pytest.mark.parametrize("name,w,h,iterations", CASES, ids=[case_key(*c) for c in CASES])
def test_reference_bits_are_the_pinned_ones(native_lib, name, w, h, iterations):
    with open(PINNED) as f:
        pinned = json.load(f)["sha256"]
    key = case_key(name, w, h, iterations)
    assert reference_digest(name, w, h, iterations) == pinned[key], key


def test_every_pinned_case_is_checked():
    with open(PINNED) as f:
        assert sorted(json.load(f)["sha256"]) == sorted(case_key(*c) for c in CASES)


if __name__ == "__main__" and sys.argv[1:] == ["--write"]:
    with open(PINNED, "w") as f:
        json.dump({"canonical_nan": "0x7fc00000", "sha256": {case_key(*c): reference_digest(*c) for c in CASES}}, f, indent=1)
        f.write("\n")
