"""GPU tests of the Miller loop's pieces on test-only code objects
(tools/pgen/unit_progs.ml_step_prog -> pairing_amd/lib/test/pa_gen_tml*.hsaco):
the G2 steps in both forms, ell, sqr12, mul12 and three trips of the loop on
the product's variable homes, one launch of about a thousand records per
object -- the structured records of tests/ml_step_cases.py tiled over the
waves plus seeded random ones.  Integer work: every record must equal the
DSL model of that very program and the plain reference
(tests/ml_step_ref.py).  The CPU side of the same programs and records is
tests/test_ml_steps.py, which also holds the workspace slot table."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools", "pgen"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import dsl  # noqa: E402

import ml_step_cases as cases  # noqa: E402
import ml_step_ref as ref  # noqa: E402
from test_ml_steps import OBJECTS, built  # noqa: E402

pytestmark = pytest.mark.gpu


def _launch(key, rows):
    """rows: lists of 12 canonical ABI integers -> the GPU's rows"""
    import torch
    import hipmod
    _, lanes, _, ws_slots = OBJECTS[key]
    n = len(rows)
    words = np.zeros((n, 72), dtype=np.uint64)
    for i, r in enumerate(rows):
        for k, x in enumerate(r):
            for j in range(6):
                words[i, 6 * k + j] = (x >> (64 * j)) & ((1 << 64) - 1)
    src = torch.from_numpy(words.view(np.int64)).cuda()
    out = torch.zeros_like(src)
    hipmod.launch(key, src, out, None, n, ws_slots=ws_slots, lanes=lanes)
    got = out.cpu().numpy().view(np.uint64)
    return [[sum(int(got[i, 6 * k + j]) << (64 * j) for j in range(6)) for k in range(12)] for i in range(n)]


@pytest.mark.parametrize("key", list(OBJECTS))
def test_ml_step_on_gpu(key):
    which, _, h, _ = OBJECTS[key]
    prog = built(key)[0]
    rows = cases.gpu_records()
    assert 900 <= len(rows) <= 1100
    gpu = _launch(key, rows)
    model, plain = {}, {}
    for r in rows:                      # the tiled records are computed once
        t = tuple(r)
        if t not in model:
            o = dsl.evaluate(prog, {k: r[k] for k in range(12)})
            model[t] = [o[k] for k in range(12)]
            plain[t] = ref.reference(which, r, h)
    bad = [i for i, r in enumerate(rows) if not (gpu[i] == model[tuple(r)] == plain[tuple(r)])]
    assert not bad, "%s: %d of %d records differ, first at %s" % (key, len(bad), len(rows), bad[:8])
