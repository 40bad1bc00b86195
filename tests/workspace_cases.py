"""The harness of tests/test_workspace_state.py: one `_device` entry run on a
caller workspace of exactly the queried size, in every state a caller can hand
over, with guard bands around the workspace and behind the outputs.

The contract under test (include/pairing_amd.h): the caller passes
`..._workspace_bytes(...)` bytes of anything and the entry gives the right
answer, writes nothing outside the window and its output rows, and leaves its
inputs alone.  check_entry() runs the entry once per state of STATES and
asserts all of that after every run, then that the output words do not depend
on what the workspace held.

Nothing here needs a GPU: `device` is where the buffers live, and
test_workspace_state.py runs the harness on "cpu" against fake entries that
break the contract one way each."""
import numpy as np
import torch

PATTERN = 0x5A
GUARD_BYTES = 4096
ALIGN = 256
GUARD_ROWS = 3
STATES = ("zeros", "ones", "pattern", "stale")
_FILL = {"zeros": 0x00, "ones": 0xFF, "pattern": PATTERN}


class Workspace:
    """lead guard | window of exactly `need` bytes, 256-byte aligned | tail guard, one uint8 buffer"""

    def __init__(self, need, device, guard=GUARD_BYTES):
        assert need >= 0 and guard >= GUARD_BYTES
        self.need = int(need)
        self.buf = torch.full((guard + ALIGN + self.need + guard,), PATTERN, dtype=torch.uint8, device=device)
        self.lead = guard + (-(self.buf.data_ptr() + guard)) % ALIGN
        assert (self.buf.data_ptr() + self.lead) % ALIGN == 0 and self.lead >= guard
        assert self.buf.numel() - self.lead - self.need >= guard

    @property
    def window(self):
        """the `need` bytes the entry may use, and not one more"""
        return self.buf[self.lead:self.lead + self.need]

    def words(self):
        """the window as int64 words, for the wrappers that count in words"""
        assert self.need % 8 == 0, "a workspace counted in words has a byte size that is a multiple of 8"
        return self.window.view(torch.int64)

    def fill(self, byte):
        self.window.fill_(byte)

    def guard_errors(self):
        """which guard bytes are no longer PATTERN, as text; empty when both bands are whole"""
        out = []
        for name, band, base in (("lead", self.buf[:self.lead], -self.lead),
                                 ("tail", self.buf[self.lead + self.need:], self.need)):
            bad = torch.nonzero(band != PATTERN).flatten()
            if bad.numel():
                out.append("%s guard of the workspace: %d bytes overwritten, the first at window offset %d"
                           % (name, bad.numel(), base + int(bad[0])))
        return out


class Output:
    """rows x width real rows followed by GUARD_ROWS guard rows, every byte PATTERN before a run"""

    def __init__(self, rows, width, dtype, device):
        self.rows = int(rows)
        self.full = torch.empty((self.rows + GUARD_ROWS, int(width)), dtype=dtype, device=device)
        self.reset()

    def reset(self):
        self.full.view(torch.uint8).fill_(PATTERN)

    def real(self):
        return _host(self.full[:self.rows])

    def guard_ok(self):
        return bool((self.full[self.rows:].contiguous().view(torch.uint8) == PATTERN).all())


def _host(t):
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a.copy()


def _snapshot(inputs):
    """host copies of every tensor and array among the inputs (handles and sizes are skipped)"""
    snap = {}
    for name, v in inputs.items():
        if isinstance(v, torch.Tensor):
            snap[name] = _host(v).copy()
        elif isinstance(v, np.ndarray):
            snap[name] = v.copy()
    return snap


def _current(v):
    return _host(v) if isinstance(v, torch.Tensor) else v


def _sync(device):
    """wait for the entry; a device fault ends the whole session, so that nothing more is started on a
    device that has faulted"""
    if torch.device(device).type != "cuda":
        return
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        import pytest
        pytest.exit("device fault while waiting for an entry, nothing more is run: %s" % e, returncode=3)


def make_outputs(spec, device):
    """{name: (rows, width, torch dtype)} -> {name: Output}"""
    return {name: Output(r, w, dt, device) for name, (r, w, dt) in spec.items()}


def check_entry(call, need_bytes, make_inputs, reference, outputs, device="cuda", equal=None, same_words=True,
                null_workspace=False, states=STATES, label="entry"):
    """Run one entry in every workspace state and assert its contract.

    call(inputs, outs, ws): enqueue the entry.  `inputs` is what make_inputs returned, `outs` maps a
        name to the full output tensor (real rows, then guard rows), `ws` is a uint8 tensor of exactly
        `need_bytes` bytes inside the guarded buffer, or None on the NULL-workspace path.
    need_bytes: what the entry's own query returns at the shape of the main inputs.  It must be > 0,
        or the case proves nothing; a case for an entry whose query is 0 says null_workspace=True and
        the entry gets no workspace at all.  An entry with several scratch buffers (the fixed-base
        table and its workspace) gives {name: bytes} and gets {name: window}; every buffer is in
        the same state and has its own guards.
    make_inputs(which): the inputs as a dict, for which = "main" and, with other seeds, "stale".  The
        stale inputs are those of the predecessor whose leftovers the `stale` state runs on; their
        plan must fit in need_bytes.  Tensors and arrays among them are compared after every run.
    reference(inputs): {output name: expected real rows (numpy)} for the given inputs, called once
        for "main" and once for "stale".
    outputs(inputs): {name: (rows, width, dtype)}.
    equal: {name: function(got, want) -> bool} where equality is not word for word (MSM sums are
        equal as points); such a case still has to give the same words in every state unless
        same_words is False.
    Returns {state: {name: real rows}}."""
    equal = equal or {}
    single = not isinstance(need_bytes, dict)
    needs = {"ws": need_bytes} if single else dict(need_bytes)
    for name, need in needs.items():
        if null_workspace:
            assert need == 0, "%s: the NULL-workspace path is for a query that returns 0, got %d" % (label, need)
        else:
            assert need > 0, "%s: the query for '%s' returned %d: the case proves nothing" % (label, name, need)
    spaces = {name: Workspace(need, device) for name, need in needs.items()}
    windows = {name: None if null_workspace else w.window for name, w in spaces.items()}
    for name, w in windows.items():
        assert w is None or (w.numel() == needs[name] and w.data_ptr() % ALIGN == 0)
    window = windows["ws"] if single else windows

    def fill(byte):
        for w in spaces.values():
            w.fill(byte)

    def run(inputs, want, state):
        outs = make_outputs(outputs(inputs), device)
        before = _snapshot(inputs)
        _sync(device)
        call(inputs, {name: o.full for name, o in outs.items()}, window)
        _sync(device)
        where = "%s, state '%s'" % (label, state)
        got = {name: o.real() for name, o in outs.items()}
        for name, exp in want.items():
            same = equal[name](got[name], exp) if name in equal else np.array_equal(got[name], exp)
            assert same, "%s: output '%s' differs from the reference" % (where, name)
        errors = ["%s ('%s')" % (e, name) for name, w in spaces.items() for e in w.guard_errors()]
        assert not errors, "%s: %s" % (where, "; ".join(errors))
        for name, o in outs.items():
            assert o.guard_ok(), "%s: the guard rows behind output '%s' were written" % (where, name)
        for name, exp in before.items():
            assert np.array_equal(_current(inputs[name]), exp), "%s: input '%s' was changed" % (where, name)
        return got

    main = make_inputs("main")
    want = reference(main)
    results = {}
    for state in states:
        if state == "stale":
            fill(PATTERN)
            prev = make_inputs("stale")
            run(prev, reference(prev), "stale (the predecessor, on a 0x5A window)")
        else:
            fill(_FILL[state])
        results[state] = run(main, want, state)
    first = results[states[0]]
    for state in states[1:]:
        for name in first:
            if same_words or name not in equal:
                assert np.array_equal(results[state][name], first[name]), \
                    "%s: the words of output '%s' differ between the states '%s' and '%s': the result depends on " \
                    "what the workspace held" % (label, name, states[0], state)
    return results
