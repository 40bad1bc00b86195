"""The environment variables the library reads are the ones INTEGRATION.md's knob
table lists, and the A/B switches that were retired with their kernel variants
stay retired: a stray variable in a service's environment must not select
another kernel, let alone change a result."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pairing_amd", "csrc")

# getenv itself or one of csrc/env.h's parsers, with the name as a literal
READ = re.compile(r'\b(?:getenv|env_clamp|env_count|env_within|env_flag)\(\s*"(PA_[A-Z0-9_]+)"')

RETIRED = (
    "PA_FQ_VARIANT", "PA_PAIRING_FIXUP", "PA_PAIRING_ML", "PA_ML_PREPARED", "PA_TAIL_SERIAL",
    "PA_WX_MUL", "PA_WX_SCAN4", "PA_WX_RADIX4", "PA_WX_SORT",
    "PA_MSM_G2_LAZY", "PA_MSM_HORNER", "PA_MSM_ACC", "PA_MSM_SERIAL", "PA_MSM_PRIO", "PA_MSM_GROUP",
    "PA_COMB_SERIAL",
)


def _text(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _names_read():
    names = set()
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".h", ".hip")):
            names.update(READ.findall(_text(os.path.join(CSRC, name))))
    return names


def _names_documented():
    doc = _text(os.path.join(ROOT, "INTEGRATION.md"))
    section = doc[doc.index("## Tuning knobs"):]
    rows = [line for line in section.splitlines() if line.startswith("|")]
    assert rows and rows[0].startswith("| knob"), "the knob table follows the heading"
    # the first cell of every row under the header and its rule
    return set(re.findall(r"PA_[A-Z0-9_]+", " ".join(r.split("|")[1] for r in rows[2:])))


def test_every_getenv_has_a_literal_name():
    """the collection below sees every read: no name reaches getenv through a variable
    (csrc/env.h passes its parameter on)"""
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".h", ".hip")) or name == "env.h":
            continue
        src = _text(os.path.join(CSRC, name))
        assert len(re.findall(r"\bgetenv\(", src)) == len(re.findall(r'\bgetenv\(\s*"PA_', src)), name


def test_knob_table_lists_what_the_library_reads():
    read, documented = _names_read(), _names_documented()
    assert read, "no knob found: the pattern no longer matches the source"
    assert read == documented, (sorted(read - documented), sorted(documented - read))


def test_retired_switches_are_gone():
    assert not set(RETIRED) & _names_read()
    pattern = re.compile(r"\b(?:%s)\b" % "|".join(RETIRED))
    me = os.path.abspath(__file__)
    hits = []
    for top in ("pairing_amd", "include", "tools", "tests"):
        for dirpath, dirnames, filenames in os.walk(os.path.join(ROOT, top)):
            dirnames[:] = [d for d in dirnames if d != "__pycache__"]
            for name in filenames:
                path = os.path.join(dirpath, name)
                if os.path.abspath(path) == me or name.endswith((".pyc", ".npz", ".so", ".o", ".hsaco")):
                    continue
                for m in pattern.finditer(_text(path)):
                    hits.append((os.path.relpath(path, ROOT), m.group(0)))
    assert not hits, hits
