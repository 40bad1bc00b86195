"""Every `_device` entry that takes a caller workspace, run on a workspace of exactly
the queried size that is zeroed, all ones, a 0x5A pattern, and left over from a
run of the same entry on other inputs (tests/workspace_cases.py: guards around the
workspace, guard rows behind the outputs, the inputs compared, the output words
the same in all four states).  The references are the ones each entry's own test
uses: the oracle's sums as points for the multiexps, bit for bit the Python
references for the transforms and the Groth16 entries.

The harness itself is tested on the CPU against fake entries that break the
contract one way each.

Where a query returns 0 the entry takes no workspace at all, and the case says so:
a one-pass transform, and r1cs_eval over the chunk system of
tests/test_groth16_setup.py, whose rows (at most six terms) stay far below
R1CS_CHUNK_LEN: its long rows are those of the transposed matrices, which
groth16_generate sums over.  r1cs_eval's chunk sums are reached by the long rows of
tests/test_r1cs.py instead."""
import numpy as np
import pytest
import torch

import decode_cases as D
import groth16_aggregate_ref as A
import groth16_ref as G
import groth16_setup_ref as S
import groth16_verify_ref as V
from helpers import R_ORDER, from_limbs, limbs, random_scalars, rng, set_infinity, small_scalars
from test_fr_ntt import MODES, inputs as fr_inputs, mont_rows, ref_ntt
from test_fr_ntt_quotient import ref_quotient, triple
from test_groth16_setup import chunk_system, gens
from test_groth16_verify import pool, real  # noqa: F401  (fixtures)
from test_msm import edge_scalars
from test_msm_prepared import wide_scalars
from workspace_cases import GUARD_ROWS, PATTERN, STATES, Workspace, check_entry

NT = 8
I64, U8 = torch.int64, torch.uint8


# ---------------- CPU: the harness catches what it is there for ----------------

def _fake_inputs(which):
    g = rng(1 if which == "main" else 2)
    return {"a": torch.from_numpy(g.integers(0, 1 << 62, size=(5, 4), dtype=np.int64)),
            "b": torch.from_numpy(g.integers(0, 1 << 62, size=(5, 4), dtype=np.int64))}


def _fake_reference(inp):
    return {"out": (inp["a"] + inp["b"]).numpy().view(np.uint64)}


def _fake_outputs(inp):
    return {"out": (5, 4, I64)}


def _fake_correct(inp, outs, ws):
    """a + b through the workspace: every cell it reads it wrote first"""
    cells = ws.view(I64)[:20].view(5, 4)
    cells.copy_(inp["a"])
    outs["out"][:5] = cells + inp["b"]


def _fake_reads_unwritten(inp, outs, ws):
    """adds a workspace cell nobody wrote: right on zeroed memory only"""
    _fake_correct(inp, outs, ws)
    outs["out"][:5] += ws.view(I64)[20]


def _fake_writes_past_the_end(inp, outs, ws):
    """one byte at `need`"""
    _fake_correct(inp, outs, ws)
    torch.as_strided(ws, (ws.numel() + 1,), (1,))[ws.numel()] = 0


def _fake_writes_before_the_start(inp, outs, ws):
    _fake_correct(inp, outs, ws)
    torch.as_strided(ws, (1,), (1,), ws.storage_offset() - 1)[0] = 0


def _fake_writes_output_guard(inp, outs, ws):
    _fake_correct(inp, outs, ws)
    outs["out"][5] = 0


def _fake_changes_input(inp, outs, ws):
    _fake_correct(inp, outs, ws)
    inp["b"][4, 3] += 1


def _fake_keeps_history(inp, outs, ws):
    """equal to the reference in a looser sense (up to one), but its words carry the low bit of a workspace
    cell it never wrote"""
    first = int(ws.view(I64)[20]) & 1
    _fake_correct(inp, outs, ws)
    outs["out"][:5] += first


def _run_fake(call, **kw):
    return check_entry(call, 256, _fake_inputs, _fake_reference, _fake_outputs, device="cpu", label="fake", **kw)


def test_harness_passes_a_correct_entry():
    res = _run_fake(_fake_correct)
    assert tuple(res) == STATES
    for got in res.values():
        np.testing.assert_array_equal(got["out"], _fake_reference(_fake_inputs("main"))["out"])


@pytest.mark.parametrize("fake,words", [
    (_fake_reads_unwritten, ("state 'ones'", "output 'out' differs")),
    (_fake_writes_past_the_end, ("state 'zeros'", "tail guard of the workspace", "window offset 256")),
    (_fake_writes_before_the_start, ("state 'zeros'", "lead guard of the workspace", "window offset -1")),
    (_fake_writes_output_guard, ("state 'zeros'", "guard rows behind output 'out'")),
    (_fake_changes_input, ("state 'zeros'", "input 'b' was changed")),
])
def test_harness_catches_a_broken_entry(fake, words):
    with pytest.raises(AssertionError) as e:
        _run_fake(fake)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_harness_catches_words_that_depend_on_the_workspace():
    """equal in the entry's own sense in every state (here: up to the low bit), and still a defect"""
    close = {"out": lambda got, want: bool((got - want <= 1).all())}
    with pytest.raises(AssertionError, match="differ between the states 'zeros' and 'ones'"):
        _run_fake(_fake_keeps_history, equal=close)
    _run_fake(_fake_keeps_history, equal=close, same_words=False)


def test_harness_refuses_a_case_that_proves_nothing():
    with pytest.raises(AssertionError, match="proves nothing"):
        check_entry(_fake_correct, 0, _fake_inputs, _fake_reference, _fake_outputs, device="cpu")
    with pytest.raises(AssertionError, match="NULL-workspace"):
        check_entry(_fake_correct, 8, _fake_inputs, _fake_reference, _fake_outputs, device="cpu", null_workspace=True)


def test_harness_places_the_window():
    for need in (1, 255, 256, 4097):
        w = Workspace(need, "cpu")
        assert w.window.numel() == need and w.window.data_ptr() % 256 == 0
        assert w.lead >= 4096 and w.buf.numel() - w.lead - need >= 4096
        assert bool((w.buf == PATTERN).all()) and not w.guard_errors()
    assert GUARD_ROWS >= 1


# ---------------- GPU: helpers ----------------

_REF = {}


def cached(key, make):
    """the oracle's answers, computed once per module and never written again"""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda:0")


def dev_bytes(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8)).to("cuda:0")


@pytest.fixture(scope="module")
def pdev(gpu):
    import pairing_amd.device as pdev
    return pdev


@pytest.fixture(scope="module")
def lib(gpu):
    from pairing_amd import _native
    return _native._lib


def words_of(ws):
    return ws.view(I64)


def point_eq(eq):
    return lambda got, want: bool(eq(got, want).all())


def picker(data):
    """make_inputs and reference over {"main": (inputs, want), "stale": (inputs, want)}"""
    def make_inputs(which):
        return dict(data[which][0], which=which)

    def reference(inp):
        return data[inp["which"]][1]
    return make_inputs, reference


# ---------------- GPU: the multiexps ----------------

def msm_scalars(g, n, kind):
    """random scalars, or the crowded form of test_multiexp_crowded_buckets (all equal but 50: cont, long_list and
    k_msm_long_fix); then the ten edge scalars, four zeros (empty buckets) and four 60-bit values (empty top windows)"""
    if kind == "crowded":
        s = np.repeat(random_scalars(g, 1), n, axis=0)
        s[n // 3:n // 3 + 50] = random_scalars(g, 1)
    else:
        s = random_scalars(g, n)
    if n >= 30:
        s[:10] = edge_scalars()
        s[20:24] = 0
        s[24:28] = random_scalars(g, 4, bits=60)
    return s


def msm_data(oracle, group, n, kind, seed):
    def make():
        g = rng(seed)
        gen, msm = ((oracle.g1_mul_generator, oracle.g1_multiexp) if group == 1 else
                    (oracle.g2_mul_generator, oracle.g2_multiexp))
        p = gen(random_scalars(g, n), NT)
        set_infinity(p, [11, n // 2])
        s = msm_scalars(g, n, kind)
        return p, s, msm(p, s, NT)
    return cached(("msm", group, n, kind, seed), make)


def other_kind(kind):
    return "random" if kind == "crowded" else "crowded"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "crowded"])
@pytest.mark.parametrize("group,n", [(1, 300), (1, 4099), (1, 1 << 14), (2, 200), (2, 2000)])
def test_multiexp(oracle, pdev, lib, group, n, kind):
    """4099: one sort tile and three items; 2^14: the second counting-sort pass.  The predecessor of the
    stale state is the other kind of scalars over other bases at the same n: the same plan, every region
    reused, and a crowded run's cont / long_list entries lie where a random run has none (and the
    other way round)"""
    data = {}
    for which, k, seed in (("main", kind, 9100), ("stale", other_kind(kind), 9150)):
        p, s, want = msm_data(oracle, group, n, k, seed + group)
        data[which] = ({"bases": dev(p), "scalars": dev(s)}, {"out": want})
    need = int(lib.pa_multiexp_workspace_bytes(group, n))
    check_entry(lambda inp, outs, ws: pdev.multiexp(group, inp["bases"], inp["scalars"], outs["out"], ws),
                need, *picker(data), lambda inp: {"out": (1, 18 * group, I64)},
                equal={"out": point_eq(oracle.g1_eq if group == 1 else oracle.g2_eq)},
                label="multiexp(%d) n=%d %s" % (group, n, kind))


def u128_data(oracle, n, seed):
    def make():
        g = rng(seed)
        bases = oracle.g1_mul_generator(small_scalars(G.rand_fr(g, n)), NT)
        set_infinity(bases, [3, n // 2])
        z = A.rand_z(g, n)
        for i, v in enumerate(A.Z_EDGES):          # 0, 1, 2^64 - 1, 2^64, 2^127, 2^128 - 1
            z[(5 * i + 1) % n] = v
        sums = A.sum_rows(oracle, oracle.g1_affine_mul(bases, small_scalars(z), NT))
        return bases, A.z_rows(z), oracle.g1_into_affine(sums)
    return cached(("u128", n, seed), make)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [33, 4097, 4099])
def test_multiexp_u128(oracle, pdev, lib, n):
    """4097: one item past a sort tile; 4099: the wider window (tests/test_groth16_aggregate.py).  As there,
    the sum is compared bit for bit as an affine record"""
    data = {}
    for which, seed in (("main", 9200), ("stale", 9250)):
        bases, z, want = u128_data(oracle, n, seed + n)
        data[which] = ({"bases": dev(bases), "scalars": dev(z)}, {"out": want})
    need = int(lib.pa_g1_multiexp_u128_workspace_bytes(n))
    check_entry(lambda inp, outs, ws: pdev.multiexp_u128(inp["bases"], inp["scalars"], outs["out"], ws),
                need, *picker(data), lambda inp: {"out": (1, 18, I64)},
                equal={"out": lambda got, want: np.array_equal(oracle.g1_into_affine(got), want)},
                label="multiexp_u128 n=%d" % n)


def prepared_bases(oracle, group, m, plan):
    """m bases in the subgroup with an infinity among them (the GLV plan), or with one curve point outside the
    subgroup (the fallback plan)"""
    def make():
        g = rng(9300 + 10 * group + m)
        gen = oracle.g1_mul_generator if group == 1 else oracle.g2_mul_generator
        p = gen(random_scalars(g, m), NT)
        set_infinity(p, [11, m // 2])
        return p
    p = cached(("prepared bases", group, m), make)
    if plan == "fallback":
        pts, truth = D.subgroup_points(group, seed=371 if group == 1 else 571, n=1)
        assert not truth[0]
        p = p.copy()
        p[137] = np.array(D.aff_record(group, pts[0]), np.uint64)
    return p


def prepared_scalars(oracle, group, p, plan, kind, seed):
    def make():
        g = rng(seed)
        s = msm_scalars(g, p.shape[0], kind)
        s[p.shape[0] // 2 + 1:p.shape[0] // 2 + 41] = wide_scalars(g, 40)    # values of r and above
        return s, (oracle.g1_multiexp if group == 1 else oracle.g2_multiexp)(p, s, NT)
    return cached(("prepared", group, p.shape[0], plan, kind, seed), make)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "crowded"])
@pytest.mark.parametrize("plan", ["glv", "fallback"])
@pytest.mark.parametrize("group,m", [(1, 4099), (2, 4096), (2, 4099)])
def test_multiexp_prepared(oracle, pdev, lib, group, m, plan, kind):
    """the bases object is built once and left alone; only the workspace changes state.  The predecessor is
    the other kind of scalars over the same object"""
    p = prepared_bases(oracle, group, m, plan)
    b = (pdev.msm_prepare if group == 1 else pdev.g2_msm_prepare)(dev(p))
    try:
        assert b.len == m and b.in_subgroup == (plan == "glv")
        data = {}
        for which, k, seed in (("main", kind, 9400), ("stale", other_kind(kind), 9450)):
            s, want = prepared_scalars(oracle, group, p, plan, k, seed + group)
            data[which] = ({"scalars": dev(s)}, {"out": want})
        need = int(getattr(lib, "pa_g%d_multiexp_prepared_workspace_bytes" % group)(b.handle(), m))
        entry = pdev.multiexp_prepared if group == 1 else pdev.g2_multiexp_prepared
        check_entry(lambda inp, outs, ws: entry(b, inp["scalars"], outs["out"], ws),
                    need, *picker(data), lambda inp: {"out": (1, 18 * group, I64)},
                    equal={"out": point_eq(oracle.g1_eq if group == 1 else oracle.g2_eq)},
                    label="multiexp_prepared(%d) m=%d %s %s" % (group, m, plan, kind))
    finally:
        b.close()


def batch_data(oracle, group, p, order, seed):
    """three vectors below r in the given order of kinds, as FrRepr and as Montgomery rows, and the oracle's sums"""
    def make():
        g = rng(seed)
        m = p.shape[0]
        vecs = []
        for kind in order:
            s = np.zeros((m, 4), np.uint64) if kind == "zero" else msm_scalars(g, m, kind)
            vecs.append(small_scalars([from_limbs(x) % R_ORDER for x in s]))
        msm = oracle.g1_multiexp if group == 1 else oracle.g2_multiexp
        want = np.concatenate([msm(p, s, NT) for s in vecs])
        repr_rows = np.ascontiguousarray(np.concatenate(vecs))
        mont, ok = oracle.fr_from_repr(repr_rows)
        assert ok.all()
        return repr_rows, mont, want
    return cached(("batch", group, p.shape[0], order, seed), make)


@pytest.mark.gpu
@pytest.mark.parametrize("montgomery", [False, True])
@pytest.mark.parametrize("group,m", [(1, 1500), (2, 700)])
def test_multiexp_prepared_batch(oracle, pdev, lib, group, m, montgomery):
    """k = 3: a crowded vector, an all-zero one and a random one.  The zero vector's row is the zero point
    (z = 0; the oracle's eq says so), not the 0x5A the row held; its predecessor in the stale state is a
    crowded vector, whose buckets, continuation pieces and window sums lie where this vector has none"""
    k = 3
    p = prepared_bases(oracle, group, m, "glv")
    b = (pdev.msm_prepare if group == 1 else pdev.g2_msm_prepare)(dev(p))
    try:
        data = {}
        for which, order, seed in (("main", ("crowded", "zero", "random"), 9500),
                                   ("stale", ("random", "crowded", "zero"), 9550)):
            repr_rows, mont, want = batch_data(oracle, group, p, order, seed + group)
            data[which] = ({"scalars": dev(mont if montgomery else repr_rows)}, {"out": want})
        jw = 18 * group
        zero_row = data["main"][1]["out"][1]
        assert not zero_row[2 * jw // 3:].any()
        need = int(getattr(lib, "pa_g%d_multiexp_prepared_batch_workspace_bytes" % group)(b.handle(), m, k))
        entry = pdev.multiexp_prepared_batch if group == 1 else pdev.g2_multiexp_prepared_batch
        check_entry(lambda inp, outs, ws: entry(b, inp["scalars"], m, k, outs["out"], ws, montgomery=montgomery),
                    need, *picker(data), lambda inp: {"out": (k, jw, I64)},
                    equal={"out": point_eq(oracle.g1_eq if group == 1 else oracle.g2_eq)},
                    label="multiexp_prepared_batch(%d) montgomery=%s" % (group, montgomery))
    finally:
        b.close()


# ---------------- GPU: the transform, the quotient, the evaluation ----------------

NTT_LOG, NTT_BATCH = 11, 2


def ntt_data(oracle, mode, seed):
    def make():
        a = fr_inputs(seed, NTT_BATCH << NTT_LOG)
        return a, ref_ntt(oracle, a, NTT_LOG, mode)
    return cached(("ntt", mode, seed), make)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_fr_ntt(gpu, oracle, pdev, mode):
    """log_n = 11 is two passes under the default tile, and the workspace is what lies between them; the
    predecessor is the next mode over other rows"""
    with gpu.fr_ntt_domain(NTT_LOG) as d:
        assert d.passes == 2
        data = {}
        for which, md, seed in (("main", mode, 9600), ("stale", MODES[(MODES.index(mode) + 1) % 4], 9650)):
            a, want = ntt_data(oracle, md, seed)
            data[which] = ({"a": dev(a), "mode": md}, {"out": want})
        check_entry(lambda inp, outs, ws: pdev.fr_ntt(d, inp["a"], outs["out"], inp["mode"], workspace=words_of(ws)),
                    d.workspace_bytes(NTT_BATCH), *picker(data), lambda inp: {"out": (NTT_BATCH << NTT_LOG, 4, I64)},
                    label="fr_ntt %s" % mode)


@pytest.mark.gpu
def test_fr_ntt_one_pass_takes_no_workspace(gpu, oracle, pdev):
    """the NULL-workspace path: a one-pass domain's query is 0 and the entry gets no workspace, so there
    are no states to run it in; the output guards and the input are checked all the same"""
    k, batch = 8, 3
    a = fr_inputs(9690, batch << k)
    data = {w: ({"a": dev(a)}, {"out": ref_ntt(oracle, a, k, "forward")}) for w in ("main",)}
    with gpu.fr_ntt_domain(k) as d:
        assert d.passes == 1
        check_entry(lambda inp, outs, ws: pdev.fr_ntt(d, inp["a"], outs["out"], "forward", workspace=ws),
                    d.workspace_bytes(batch), *picker(data), lambda inp: {"out": (batch << k, 4, I64)},
                    null_workspace=True, states=("pattern",), label="fr_ntt one pass")


def quotient_data(oracle, seed):
    def make():
        a, b, c = triple(seed, NTT_BATCH << NTT_LOG)
        return a, b, c, ref_quotient(oracle, a, b, c, NTT_LOG)
    return cached(("quotient", seed), make)


@pytest.mark.gpu
@pytest.mark.parametrize("alias", [False, True])
def test_fr_ntt_quotient(gpu, oracle, pdev, alias):
    """with alias the evaluations of a are copied into the output rows and the call runs with out = a"""
    rows = NTT_BATCH << NTT_LOG
    with gpu.fr_ntt_domain(NTT_LOG) as d:
        data = {}
        for which, seed in (("main", 9700), ("stale", 9750)):
            a, b, c, want = quotient_data(oracle, seed)
            data[which] = ({"a": dev(a), "b": dev(b), "c": dev(c)}, {"out": want})

        def call(inp, outs, ws):
            out, a = outs["out"], inp["a"]
            if alias:
                out[:rows].copy_(a)
                a = out[:rows]
            pdev.fr_ntt_quotient(d, a, inp["b"], inp["c"], out, workspace=words_of(ws))
        check_entry(call, d.quotient_workspace_bytes(NTT_BATCH), *picker(data), lambda inp: {"out": (rows, 4, I64)},
                    label="fr_ntt_quotient alias=%s" % alias)


def long_rows_system(gpu):
    """the rows of test_rows_around_the_chunk_length's mixed case, shortened to what reaches the chunk sums: 0,
    1, L - 1, L, L + 1, 2 L + 1, 5 L terms among one-term rows over 40 columns (so long rows repeat columns)"""
    from test_r1cs import long_row
    L = gpu.R1CS_CHUNK_LEN
    g = rng(9800)
    n_cols = 40
    a = []
    for length in (0, 1, L - 1, L, L + 1, 2 * L + 1, 5 * L, 0, 3 * L):
        a += [long_row(g, length, n_cols), long_row(g, 1, n_cols)]
    b = [long_row(g, (7 * i) % (L + 2), n_cols) for i in range(len(a))]
    c = [long_row(g, 2 * L + 3 if i == 4 else 1, n_cols) for i in range(len(a))]
    return (a, b, c), len(a), n_cols, 5


def eval_data(mats, n_cols, log_n, k, seed):
    def make():
        g = rng(seed)
        ws = [G.rand_fr(g, n_cols) for _ in range(k)]
        return mont_rows([v for w in ws for v in w]), G.ref_eval(mats, ws, log_n)
    return cached(("eval", n_cols, log_n, k, seed), make)


@pytest.mark.gpu
@pytest.mark.parametrize("which_system", ["long_rows", "chunk_system"])
def test_r1cs_eval(gpu, oracle, pdev, which_system):
    """k = 2.  long_rows: rows over R1CS_CHUNK_LEN, whose chunk sums are the workspace.  chunk_system: duplicate
    columns and (in C) empty rows, but no row over the chunk length, so its query is 0: the NULL-workspace
    path, run once"""
    k = 2
    if which_system == "long_rows":
        mats, n_rows, n_cols, log_n = long_rows_system(gpu)
    else:
        mats, n_rows, n_cols, log_n = chunk_system(True), 64, 67, 6
    rows = k << log_n
    with gpu.r1cs(*(G.csr(m) for m in mats), n_rows, n_cols) as sysm:
        need = sysm.eval_workspace_bytes(k)
        null = which_system == "chunk_system"
        data = {}
        for which, seed in (("main", 9810), ("stale", 9815)):
            w, (a, b, c) = eval_data(mats, n_cols, log_n, k, seed + n_cols)
            data[which] = ({"witness": dev(w)}, {"a": a, "b": b, "c": c})

        def call(inp, outs, ws):
            pdev.r1cs_eval(sysm, inp["witness"], log_n, outs["a"], outs["b"], outs["c"],
                           workspace=None if ws is None else words_of(ws))
        check_entry(call, need, *picker(data), lambda inp: {n: (rows, 4, I64) for n in "abc"},
                    null_workspace=null, states=("pattern",) if null else STATES, label="r1cs_eval %s" % which_system)


# ---------------- GPU: the Groth16 entries ----------------

def real_system():
    """the real-setup system at log_n = 5 (30 rows, 12 variables, 3 public), its witness and a spoiled one"""
    def make():
        mats, w = G.satisfied_system(7100, 30, 12)
        spoiled = list(w)
        spoiled[9] = (spoiled[9] + 5) % R_ORDER
        return mats, w, spoiled
    return cached("real system", make)


def prove_data(oracle, name, key, mats, ws, seed):
    def make():
        g = rng(seed)
        rs, ss = G.rand_fr(g, len(ws)), G.rand_fr(g, len(ws))
        return (mont_rows([v for w in ws for v in w]), mont_rows(rs), mont_rows(ss),
                G.ref_proofs(oracle, key, mats, ws, rs, ss))
    return cached(("prove", name, seed), make)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["real", "chunk"])
def test_groth16_prove(gpu, oracle, pdev, name):
    """real: k = 4 over the real setup (log_n = 5), the predecessor with a spoiled witness among the four.  chunk:
    k = 2 over the chunk system (log_n = 6) under a random key, witnesses that do not satisfy it"""
    if name == "real":
        mats, w, spoiled = real_system()
        key = cached("real key", lambda: G.real_setup(7101, mats, 12, 3, 5))[0]
        n_rows, witnesses = 30, {"main": [w, w, w, w], "stale": [w, spoiled, w, spoiled]}
    else:
        mats = chunk_system(False)
        key = cached("chunk key", lambda: G.random_key(9900, 67, 4, 6, 63))
        g = rng(9901)
        n_rows = 64
        witnesses = {which: [[1] + G.rand_fr(g, 66) for _ in range(2)] for which in ("main", "stale")}
    k = len(witnesses["main"])
    pk = gpu.groth16_pk(*key.points(oracle))
    sysm = gpu.r1cs(*(G.csr(m) for m in mats), n_rows, key.n_vars)
    dom = gpu.fr_ntt_domain(key.log_n)
    try:
        data = {}
        for which, seed in (("main", 9910), ("stale", 9915)):
            w_rows, r, s, want = prove_data(oracle, name + which, key, mats, witnesses[which], seed)
            data[which] = ({"witness": dev(w_rows), "r": dev(r), "s": dev(s)}, {"out": want})
        check_entry(lambda inp, outs, ws: pdev.groth16_prove(pk, sysm, dom, inp["witness"], inp["r"], inp["s"],
                                                             outs["out"], ws),
                    pk.prove_workspace_bytes(sysm, k), *picker(data), lambda inp: {"out": (k, 51, I64)},
                    label="groth16_prove %s" % name)
    finally:
        for x in (pk, sysm, dom):
            x.close()


def setup_data(oracle, name, seed):
    def make():
        if name == "real":
            mats, shape = real_system()[0], (12, 3, 5)
        else:
            mats, shape = chunk_system(False), (67, 4, 6)
        st = S.Setup(mats, *shape, S.trapdoor_of(seed))
        return st.trapdoor_rows(), st.scalar_rows(), st.g1_points(oracle), st.g2_points(oracle)
    return cached(("setup", name, seed), make)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["real", "chunk"])
def test_groth16_generate(gpu, oracle, pdev, name):
    """both generation entries; the predecessor uses another trapdoor.  chunk: variable 0 stands in every row, so
    its transposed row folds over several chunks; variables 33 and 66 stand nowhere (infinity records)"""
    mats, n_rows, n_vars, n_public, log_n = ((real_system()[0], 30, 12, 3, 5) if name == "real" else
                                             (chunk_system(False), 64, 67, 4, 6))
    circ = gpu.groth16_circuit(*(G.csr(m) for m in mats), n_rows, n_vars, n_public)
    dom = gpu.fr_ntt_domain(log_n)
    try:
        g1, g2 = gens(oracle)
        data, sdata = {}, {}
        for which, seed in (("main", 7131), ("stale", 9925)):
            td, sc, p1, p2 = setup_data(oracle, name, seed)
            data[which] = ({"g1": dev(g1), "g2": dev(g2), "trapdoor": td}, {"g1_out": p1, "g2_out": p2})
            sdata[which] = ({"trapdoor": td}, {"out": sc})
        need = circ.generate_workspace_bytes(log_n)
        n1, n2 = circ.g1_len(log_n), circ.g2_len()
        check_entry(lambda inp, outs, ws: pdev.groth16_generate(circ, dom, inp["g1"], inp["g2"], inp["trapdoor"],
                                                                outs["g1_out"], outs["g2_out"], ws),
                    need, *picker(data), lambda inp: {"g1_out": (n1, 13, I64), "g2_out": (n2, 25, I64)},
                    label="groth16_generate %s" % name)
        check_entry(lambda inp, outs, ws: pdev.groth16_generate_scalars(circ, dom, inp["trapdoor"], outs["out"], ws),
                    need, *picker(sdata), lambda inp: {"out": (n1, 4, I64)},
                    label="groth16_generate_scalars %s" % name)
    finally:
        circ.close()
        dom.close()


# the pool of tests/test_groth16_verify.py: 0, 1 valid; 2 a spoiled witness; 3, 4, 5 one of A, B, C replaced; 6 a wrong
# public input; 7 A at infinity
VERIFY_MAIN = [0, 2, 1, 7, 4]
VERIFY_STALE = [3, 0, 5, 1, 6]


def verify_batch(pool, idx):  # noqa: F811
    return (np.ascontiguousarray(pool.proofs[idx]), np.ascontiguousarray(pool.mont[idx].reshape(-1, 4)),
            pool.gt[idx], pool.valid[idx].astype(np.uint8).reshape(-1, 1))


@pytest.mark.gpu
def test_groth16_verify(gpu, oracle, pdev, pool):  # noqa: F811
    """k = 5 with a spoiled proof and one whose A is infinity: valid and gt, the encoded entry's status, and the
    input sums alone.  valid and gt start as 0x5A, so nothing left over can pass for an answer"""
    k = 5
    vk = gpu.groth16_vk(*pool.vk.args())
    try:
        data, enc, sums = {}, {}, {}
        for which, idx in (("main", VERIFY_MAIN), ("stale", VERIFY_STALE)):
            proofs, mont, gt, valid = verify_batch(pool, idx)
            assert valid.any() and not valid.all()
            X = dev(mont)
            data[which] = ({"proofs": dev(proofs), "inputs": X}, {"valid": valid, "gt": gt})
            wire = V.encode_proofs(proofs)
            status = cached(("status", which), lambda: V.decode_status(oracle, wire))
            assert not status.any()
            enc[which] = ({"data": dev_bytes(wire), "inputs": X}, {"valid": valid, "gt": gt, "status": status})
            want = cached(("input sum", which),
                          lambda: V.ref_input_sum(oracle, pool.vk.ic, [pool.inputs[j] for j in idx]))
            sums[which] = ({"inputs": X}, {"out": want})
        need = vk.verify_workspace_bytes(k)
        check_entry(lambda inp, outs, ws: pdev.groth16_verify(vk, inp["proofs"], inp["inputs"], outs["valid"], ws,
                                                              gt=outs["gt"]),
                    need, *picker(data), lambda inp: {"valid": (k, 1, U8), "gt": (k, 72, I64)}, label="groth16_verify")
        check_entry(lambda inp, outs, ws: pdev.groth16_verify_encoded(vk, inp["data"], inp["inputs"], outs["valid"],
                                                                      outs["status"], ws, gt=outs["gt"]),
                    need, *picker(enc), lambda inp: {"valid": (k, 1, U8), "status": (k, 3, U8), "gt": (k, 72, I64)},
                    label="groth16_verify_encoded")
        check_entry(lambda inp, outs, ws: pdev.groth16_input_sum(vk, inp["inputs"], k, outs["out"], ws),
                    vk.input_sum_workspace_bytes(k), *picker(sums), lambda inp: {"out": (k, 13, I64)},
                    label="groth16_input_sum")
    finally:
        vk.close()


def aggregate_data(oracle, pool, k, good, seed):  # noqa: F811
    """k proofs tiling the pool's two valid ones, with a spoiled one in the middle unless `good`, under fixed weights"""
    def make():
        g = rng(seed)
        idx = [j % 2 for j in range(k)]
        if not good:
            idx[k // 2] = 2
        proofs = np.ascontiguousarray(pool.proofs[idx])
        inputs = [pool.inputs[j] for j in idx]
        z = [v | 1 for v in A.rand_z(g, k)]
        z[0], z[k - 1] = (1 << 128) - 1, 1 << 64
        gt, valid = A.ref_aggregate(oracle, pool.vk, proofs, inputs, z)
        assert valid == good
        return (proofs, mont_rows([x for row in inputs for x in row]), A.z_rows(z), gt,
                np.array([[int(valid)]], np.uint8), A.ref_points(oracle, pool.vk, proofs, inputs, z))
    return cached(("aggregate", k, good, seed), make)


@pytest.mark.gpu
@pytest.mark.parametrize("good", [True, False])
@pytest.mark.parametrize("k", [5, 33])
def test_groth16_verify_aggregate(gpu, oracle, pdev, pool, k, good):  # noqa: F811
    """the three aggregate entries under fixed z.  The predecessor is the batch of the other verdict, so a
    leftover verdict, weight sum or P array would be the wrong one; valid and gt start as 0x5A"""
    vk = gpu.groth16_vk(*pool.vk.args())
    try:
        data, enc, pts = {}, {}, {}
        for which, verdict, seed in (("main", good, 9940), ("stale", not good, 9945)):
            proofs, mont, z, gt, valid, points = aggregate_data(oracle, pool, k, verdict, seed + k)
            X, Z = dev(mont), dev(z)
            data[which] = ({"proofs": dev(proofs), "inputs": X, "z": Z}, {"valid": valid, "gt": gt})
            enc[which] = ({"data": dev_bytes(V.encode_proofs(proofs)), "inputs": X, "z": Z},
                          {"valid": valid, "gt": gt, "status": np.zeros((k, 3), np.uint8)})
            pts[which] = ({"proofs": dev(proofs), "inputs": X, "z": Z}, {"out": points})
        need = vk.verify_aggregate_workspace_bytes(k)
        label = " k=%d %s" % (k, "valid" if good else "spoiled")
        check_entry(lambda inp, outs, ws: pdev.groth16_verify_aggregate(vk, inp["proofs"], inp["inputs"], inp["z"],
                                                                        outs["valid"], ws, gt=outs["gt"]),
                    need, *picker(data), lambda inp: {"valid": (1, 1, U8), "gt": (1, 72, I64)},
                    label="groth16_verify_aggregate" + label)
        check_entry(lambda inp, outs, ws: pdev.groth16_verify_aggregate_encoded(
                        vk, inp["data"], inp["inputs"], inp["z"], outs["valid"], outs["status"], ws, gt=outs["gt"]),
                    need, *picker(enc), lambda inp: {"valid": (1, 1, U8), "status": (k, 3, U8), "gt": (1, 72, I64)},
                    label="groth16_verify_aggregate_encoded" + label)
        check_entry(lambda inp, outs, ws: pdev.groth16_aggregate_points(vk, inp["proofs"], inp["inputs"], inp["z"],
                                                                        outs["out"], ws),
                    need, *picker(pts), lambda inp: {"out": (k + 3, 13, I64)}, label="groth16_aggregate_points" + label)
    finally:
        vk.close()


# ---------------- GPU: the wNAF entries, the comb buffers, the pairings ----------------

@pytest.mark.gpu
@pytest.mark.parametrize("group", [1, 2])
def test_wnaf_exact(oracle, pdev, lib, group):
    """window 6: 100 scalars under one base (the table and the digit columns), and 5 bases under one scalar (a
    table per base); the reference's Jacobian words"""
    from test_wnaf_exact import _edge_scalars, _g1_base, _g2_base
    jw = 18 * group
    ofb = oracle.g1_wnaf_fixed_base if group == 1 else oracle.g2_wnaf_fixed_base
    mkbase = _g1_base if group == 1 else _g2_base
    fb, fs = {}, {}
    for which, seed in (("main", 9950), ("stale", 9955)):
        base = mkbase(oracle, seed + group)
        s = _edge_scalars(rng(seed + 2 + group), 100)
        fb[which] = ({"base": dev(base), "scalars": dev(s)},
                     {"out": cached(("wnaf fb", group, which), lambda: ofb(base, s, NT, window=6))})
        bases = np.ascontiguousarray(np.concatenate([mkbase(oracle, seed + 10 * i + group) for i in range(5)]))
        one = np.ascontiguousarray(s[40 if which == "main" else 7:][:1])
        want = cached(("wnaf fs", group, which), lambda: np.concatenate(
            [ofb(np.ascontiguousarray(bases[i:i + 1]), one, 1, window=6) for i in range(5)]))
        fs[which] = ({"bases": dev(bases), "scalar": dev(one)}, {"out": want})
    check_entry(lambda inp, outs, ws: pdev.wnaf_fixed_base_exact(group, inp["base"], inp["scalars"], outs["out"], 6, ws),
                int(lib.pa_wnaf_exact_workspace_bytes(group, 100, 6, 0)), *picker(fb),
                lambda inp: {"out": (100, jw, I64)}, label="wnaf_fixed_base_exact(%d)" % group)
    check_entry(lambda inp, outs, ws: pdev.wnaf_fixed_scalar_exact(group, inp["bases"], inp["scalar"], outs["out"], 6, ws),
                int(lib.pa_wnaf_exact_workspace_bytes(group, 5, 6, 1)), *picker(fs),
                lambda inp: {"out": (5, jw, I64)}, label="wnaf_fixed_scalar_exact(%d)" % group)


def halves_scalars(g, n, wrap=True):
    """test_g1_fixed_base_overlapped_halves' digit edges among random scalars; the last one, 2^256 - 1, is
    where wnaf_form wraps: the G1 entry's test pins it, the G2 entry's has 128 + 256 * 128 in its place"""
    s = random_scalars(g, n)
    for i, v in enumerate([0, 1, R_ORDER - 1, (1 << 255) - 1, 1 << 200, (1 << 130) - 1, 0x80 << 128, 0x81 << 128,
                           (1 << 256) - 1 if wrap else 128 + 256 * 128]):
        s[i] = limbs(v, 4)
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("group", [1, 2])
def test_wnaf_fixed_base_buffers(oracle, pdev, lib, group):
    """g{1,2}_wnaf_fixed_base build their table in the same call: table and ws are both scratch here, both in
    every state and both guarded; 300 scalars, equal as points to the reference's wNAF (as the entries' own
    tests compare them)"""
    jw = 18 * group
    n = 300
    ofb, eq, entry = ((oracle.g1_wnaf_fixed_base, oracle.g1_eq, pdev.g1_wnaf_fixed_base) if group == 1 else
                      (oracle.g2_wnaf_fixed_base, oracle.g2_eq, pdev.g2_wnaf_fixed_base))
    data = {}
    for which, seed in (("main", 9960), ("stale", 9965)):
        g = rng(seed + group)
        if group == 1:
            base = oracle.g1_mul_generator_jacobian(random_scalars(g, 1))
        else:
            base = oracle.g2_from_affine(oracle.g2_mul_generator(random_scalars(g, 1)))
        s = halves_scalars(g, n, wrap=group == 1)
        data[which] =({"base": dev(base), "scalars": dev(s)},
                       {"out": cached(("comb", group, which), lambda: ofb(base, s, NT))})
    need = {"table": 8 * int(getattr(lib, "pa_g%d_fixed_base_table_words" % group)()),
            "ws": 8 * int(getattr(lib, "pa_g%d_fixed_base_workspace_words" % group)())}
    check_entry(lambda inp, outs, ws: entry(inp["base"], inp["scalars"], outs["out"], words_of(ws["table"]),
                                            words_of(ws["ws"])),
                need, *picker(data), lambda inp: {"out": (n, jw, I64)}, equal={"out": point_eq(eq)},
                label="g%d_wnaf_fixed_base" % group)


@pytest.mark.gpu
def test_g1_fixed_base_table_then_mul(oracle, pdev, lib):
    """the comb table is an input of the second call and no scratch: it is built on dirtied buffers (table
    and ws 0xFF), then left alone, and g1_fixed_base_mul reads it"""
    g = rng(9970)
    base = oracle.g1_mul_generator_jacobian(random_scalars(g, 1))
    s = halves_scalars(g, 300)
    s[[3, 8]] = random_scalars(g, 2)     # below r only: there s * base means one thing
    want = oracle.g1_wnaf_fixed_base(base, s, NT)
    from pairing_amd.device import _stream_ptr, call
    import ctypes
    B, S_ = dev(base), dev(s)
    table =Workspace(8 * int(lib.pa_g1_fixed_base_table_words()), "cuda:0")
    ws = Workspace(8 * int(lib.pa_g1_fixed_base_workspace_words()), "cuda:0")
    assert table.need > 0 and ws.need > 0
    table.fill(0xFF)
    ws.fill(0xFF)
    call("pa_g1_fixed_base_table_device", ctypes.c_void_p(B.data_ptr()),
         ctypes.c_void_p(table.window.data_ptr()), ctypes.c_void_p(ws.window.data_ptr()), _stream_ptr(None))
    torch.cuda.synchronize()
    ws.fill(0x00)      # the build's workspace is free again; the table is not touched
    out = torch.full((300 + GUARD_ROWS, 18), 0x5A5A5A5A5A5A5A5A, dtype=I64, device="cuda:0")
    pdev.g1_fixed_base_mul(words_of(table.window), S_, out)
    torch.cuda.synchronize()
    host = out.cpu().numpy().view(np.uint64)
    assert oracle.g1_eq(host[:300], want).all()
    assert (host[300:] == 0x5A5A5A5A5A5A5A5A).all()
    assert not table.guard_errors() and not ws.guard_errors()


def pairs9(seed):
    import bench
    p, q = bench.make_pairs(9, 0, seed=seed)
    set_infinity(p, [4])
    return p, q


@pytest.mark.gpu
def test_pairing_scratch_and_multi_pairing_work(oracle, pdev):
    """9 pairs, one with P at infinity.  Neither entry has a size query: the header gives n Fq12 rows for
    `scratch` and `work`"""
    from test_multi_pairing_batch import _expected
    n = 9
    pair, multi = {}, {}
    for which, seed in (("main", 9980), ("stale", 9985)):
        p, q = pairs9(seed)
        P, Q = dev(p), dev(q)
        pair[which] = ({"p": P, "q": Q}, {"out": cached(("pairing", which), lambda: oracle.pairing(p, q, 4))})
        out, ok, _ = cached(("multi", which), lambda: _expected(oracle, p, q, np.array([0, n], np.uint64)))
        multi[which] = ({"p": P, "q": Q}, {"out": out, "ok": np.asarray(ok, np.uint8).reshape(1, 1)})
    need = n * 72 * 8
    rows = lambda ws: words_of(ws).view(n, 72)   # noqa: E731
    check_entry(lambda inp, outs, ws: pdev.pairing(inp["p"], inp["q"], outs["out"], rows(ws)),
                need, *picker(pair), lambda inp: {"out": (n, 72, I64)}, label="pairing")
    check_entry(lambda inp, outs, ws: pdev.multi_pairing(inp["p"], inp["q"], outs["out"], outs["ok"], rows(ws)),
                need, *picker(multi), lambda inp: {"out": (1, 72, I64), "ok": (1, 1, U8)}, label="multi_pairing")


# ---------------- GPU: one buffer through the chain ----------------

@pytest.mark.gpu
def test_one_workspace_through_generate_prove_verify_aggregate(gpu, oracle, pdev):
    """one buffer of the largest size any stage asks for, filled with 0xFF once and never again: generate ->
    keys -> prove (k = 4) -> verify -> aggregate -> prove other witnesses under other r, s -> verify, every
    stage against its reference and the guards checked after each"""
    from pairing_amd._native import Groth16Params
    mats, w, spoiled = real_system()
    k, n_vars, n_public, log_n = 4, 12, 3, 5
    st = S.Setup(mats, n_vars, n_public, log_n, S.trapdoor_of(7101))
    key = G.Key(st.alpha, st.beta, st.delta, st.u, st.v, st.l, st.h, n_public, log_n)
    g = rng(9990)
    circ = gpu.groth16_circuit(*(G.csr(m) for m in mats), 30, n_vars, n_public)
    sysm = gpu.r1cs(*(G.csr(m) for m in mats), 30, n_vars)
    dom = gpu.fr_ntt_domain(log_n)
    closing = [circ, sysm, dom]
    try:
        n1, n2 = circ.g1_len(log_n), circ.g2_len()
        g1, g2 = gens(oracle)
        o1 = torch.full((n1, 13), 0x5A5A5A5A5A5A5A5A, dtype=I64, device="cuda:0")
        o2 = torch.full((n2, 25), 0x5A5A5A5A5A5A5A5A, dtype=I64, device="cuda:0")
        # the keys' sizes do not depend on the trapdoor: one built from the reference's points tells every need
        sizing_pk = gpu.groth16_pk(*key.points(oracle))
        vkp = V.vk_from_ints(oracle, st.alpha, st.beta, st.gamma, st.delta, st.ic)
        sizing_vk = gpu.groth16_vk(*vkp.args())
        needs = [circ.generate_workspace_bytes(log_n), sizing_pk.prove_workspace_bytes(sysm, k),
                 sizing_vk.verify_workspace_bytes(k), sizing_vk.verify_aggregate_workspace_bytes(k)]
        sizing_pk.close()
        sizing_vk.close()
        assert min(needs) > 0
        space = Workspace(max(needs), "cuda:0")
        space.fill(0xFF)
        ws = space.window

        def guards(stage):
            torch.cuda.synchronize()
            errors = space.guard_errors()
            assert not errors, "%s: %s" % (stage, "; ".join(errors))

        pdev.groth16_generate(circ, dom, dev(g1), dev(g2), st.trapdoor_rows(), o1, o2, ws)
        guards("generate")
        h1, h2 = o1.cpu().numpy().view(np.uint64), o2.cpu().numpy().view(np.uint64)
        np.testing.assert_array_equal(h1, st.g1_points(oracle))
        np.testing.assert_array_equal(h2, st.g2_points(oracle))
        params = Groth16Params(h1, h2, n_vars, n_public, log_n)
        pk, vk = gpu.groth16_pk(*params.pk_args()), gpu.groth16_vk(*params.vk_args())
        closing += [pk, vk]
        assert needs[1] == pk.prove_workspace_bytes(sysm, k) and needs[2] == vk.verify_workspace_bytes(k)

        z = [v | 1 for v in A.rand_z(g, k)]
        Z = dev(A.z_rows(z))
        for round_, witnesses, want_valid in (("first", [w, w, spoiled, w], [1, 1, 0, 1]),
                                              ("second", [spoiled, w, w, w], [0, 1, 1, 1])):
            rs, ss = G.rand_fr(g, k), G.rand_fr(g, k)
            W = dev(mont_rows([x for v in witnesses for x in v]))
            proofs = torch.full((k, 51), 0x5A5A5A5A5A5A5A5A, dtype=I64, device="cuda:0")
            pdev.groth16_prove(pk, sysm, dom, W, dev(mont_rows(rs)), dev(mont_rows(ss)), proofs, ws)
            guards(round_ + " prove")
            host = proofs.cpu().numpy().view(np.uint64)
            np.testing.assert_array_equal(host, G.ref_proofs(oracle, key, mats, witnesses, rs, ss), err_msg=round_)
            valid = torch.full((k,), PATTERN, dtype=U8, device="cuda:0")
            gt = torch.full((k, 72), 0x5A5A5A5A5A5A5A5A, dtype=I64, device="cuda:0")
            pdev.groth16_verify(vk, proofs, W[1:], valid, ws, gt=gt, stride=n_vars)
            guards(round_ + " verify")
            inputs = [list(v[1:n_public]) for v in witnesses]
            want_gt, want = V.ref_verify(oracle, vkp, host, inputs)
            assert valid.cpu().tolist() == want_valid == want.astype(int).tolist(), round_
            np.testing.assert_array_equal(gt.cpu().numpy().view(np.uint64), want_gt, err_msg=round_)
            if round_ == "first":
                one = torch.full((1,), PATTERN, dtype=U8, device="cuda:0")
                agt = torch.full((1, 72), 0x5A5A5A5A5A5A5A5A, dtype=I64, device="cuda:0")
                pdev.groth16_verify_aggregate(vk, proofs, W[1:], Z, one, ws, gt=agt, stride=n_vars)
                guards("aggregate")
                want_agt, want_one = A.ref_aggregate(oracle, vkp, host, inputs, z)
                assert one.cpu().tolist() == [int(want_one)] == [0]
                np.testing.assert_array_equal(agt.cpu().numpy().view(np.uint64), want_agt)
    finally:
        for x in closing:
            x.close()


# ---------------- GPU: the host entries keep their buffers between calls ----------------

@pytest.mark.gpu
def test_host_entries_keep_buffers_between_calls(gpu, oracle, pool):  # noqa: F811
    """each host entry once at the larger shape with one seed, then at the smaller shape with another, in this
    process and on this thread: whatever the first call left in a buffer the entry keeps, the second result is
    its reference's"""
    # the multiexps
    for group, big, small_n in ((1, 1 << 14, 300), (2, 2000, 200)):
        msm, eq = (gpu.g1_multiexp, oracle.g1_eq) if group == 1 else (gpu.g2_multiexp, oracle.g2_eq)
        p, s, want = msm_data(oracle, group, big, "crowded", 9100 + group)
        assert eq(msm(p, s), want).all()
        p, s, want = msm_data(oracle, group, small_n, "random", 9100 + group)
        assert eq(msm(p, s), want).all(), "g%d_multiexp after a larger call" % group
    for n, seed in ((4099, 9200), (33, 9250)):
        bases, z, want = u128_data(oracle, n, seed + n)
        np.testing.assert_array_equal(oracle.g1_into_affine(gpu.g1_multiexp_u128(bases, z)), want)
    for m, order, seed in ((1500, ("crowded", "zero", "random"), 9500), (300, ("random", "crowded", "zero"), 9560)):
        p = prepared_bases(oracle, 1, m, "glv")
        repr_rows, _, want = batch_data(oracle, 1, p, order, seed + 1)
        with gpu.g1_msm_prepare(p) as b:
            assert oracle.g1_eq(gpu.g1_multiexp_prepared_batch(b, repr_rows, count=3), want).all(), m
    # the transform and the quotient: log_n = 11, batch 2, then log_n = 9, batch 1
    with gpu.fr_ntt_domain(NTT_LOG) as d:
        a, want = ntt_data(oracle, "coset_forward", 9600)
        np.testing.assert_array_equal(gpu.fr_ntt(d, a, "coset_forward"), want)
        a, b, c, want = quotient_data(oracle, 9700)
        np.testing.assert_array_equal(gpu.fr_ntt_quotient(d, a, b, c), want)
    with gpu.fr_ntt_domain(9) as d:
        a = fr_inputs(9995, 1 << 9)
        np.testing.assert_array_equal(gpu.fr_ntt(d, a, "inverse"), ref_ntt(oracle, a, 9, "inverse"))
        a, b, c = triple(9996, 1 << 9)
        np.testing.assert_array_equal(gpu.fr_ntt_quotient(d, a, b, c), ref_quotient(oracle, a, b, c, 9))
    # the prover: the chunk system (log_n = 6, k = 2), then the real one (log_n = 5, k = 1)
    mats = chunk_system(False)
    key = cached("chunk key", lambda: G.random_key(9900, 67, 4, 6, 63))
    g = rng(9997)
    for mats, key, n_rows, witnesses in (
            (mats, key, 64, [[1] + G.rand_fr(g, 66) for _ in range(2)]),
            (real_system()[0], cached("real key", lambda: G.real_setup(7101, real_system()[0], 12, 3, 5))[0], 30,
             [real_system()[1]])):
        rs, ss = G.rand_fr(g, len(witnesses)), G.rand_fr(g, len(witnesses))
        pk = gpu.groth16_pk(*key.points(oracle))
        sysm = gpu.r1cs(*(G.csr(m) for m in mats), n_rows, key.n_vars)
        dom = gpu.fr_ntt_domain(key.log_n)
        try:
            got = gpu.groth16_prove(pk, sysm, dom, mont_rows([v for w in witnesses for v in w]), mont_rows(rs),
                                    mont_rows(ss))
            np.testing.assert_array_equal(got, G.ref_proofs(oracle, key, mats, witnesses, rs, ss))
        finally:
            for x in (pk, sysm, dom):
                x.close()
    # the verifiers: k = 33, then k = 5 of the other verdict
    with gpu.groth16_vk(*pool.vk.args()) as vk:
        for k, good in ((33, True), (5, False)):
            proofs, mont, z, gt, valid, _ = aggregate_data(oracle, pool, k, good, 9940 + k)
            got_valid, got_gt = gpu.groth16_verify_aggregate(vk, proofs, mont, z, return_gt=True)
            assert got_valid is good
            np.testing.assert_array_equal(got_gt, gt)
        for idx in (list(range(8)) * 4 + [0], VERIFY_MAIN):
            proofs, mont, gt, valid = verify_batch(pool, idx)
            got_valid, got_gt = gpu.groth16_verify(vk, proofs, mont, return_gt=True)
            np.testing.assert_array_equal(got_valid, valid[:, 0].astype(bool))
            np.testing.assert_array_equal(got_gt, gt)
