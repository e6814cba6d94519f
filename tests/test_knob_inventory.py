"""The knob list (tests/knob_table.py) against the sources: every UGP_* environment variable the library reads has exactly one
row, each row's test file names the knob, and a knob read while flattening is either hashed into flat_signature() or says why
a flat file written without it stays correct.  CPU only: reads source text."""
import os
import re

from tests import knob_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "usher_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")
GRID_FILE = "test_knobs_gpu.py"

# a string literal, or a comment: comments are dropped, strings kept (a name that appears only in a comment is no knob)
_TOKENS = re.compile(r'"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'|//[^\n]*|/\*.*?\*/', re.S)
# a read of the environment: getenv("UGP_..."), or one of the Knobs helpers flag / num / pos (ugp_knobs.hpp)
_READ = re.compile(r'\b(?:getenv|flag|num|pos)\(\s*"(UGP_[A-Z0-9_]+)"')


def _strip_comments(text):
    return _TOKENS.sub(lambda m: m.group(0) if m.group(0)[0] in "\"'" else " ", text)


def _sources():
    out = {}
    for d, _, files in os.walk(CSRC):
        for f in sorted(files):
            if f.endswith((".hpp", ".cpp", ".hip", ".h")):
                p = os.path.join(d, f)
                with open(p) as fh:
                    out[os.path.relpath(p, CSRC)] = _strip_comments(fh.read())
    return out


def _reads(text):
    return set(_READ.findall(text))


def _body(text, head):
    """The text of the function whose definition starts with `head`, up to its closing brace at column 0."""
    i = text.index(head)
    j = text.index("\n}\n", i)
    return text[i:j]


def _signature_names(capi):
    body = _body(capi, "uint64_t flat_signature()")
    m = re.search(r'for\s*\(\s*const\s+char\s*\*\s*k\s*:\s*\{(.*?)\}\s*\)', body, re.S)
    assert m, "flat_signature() no longer lists its switches in one `for (const char *k : {...})`"
    return set(re.findall(r'"(UGP_[A-Z0-9_]+)"', m.group(1)))


def _flatten_reads(src):
    """Names read while a tree is flattened: the flattening itself, the coarse tree, the flattening options."""
    capi = src["ugp_capi.cpp"]
    names = _reads(src["ugp_flatten.cpp"])
    for head in ("static ugp::Options default_options()", "static int build_coarse(", "static int mat_create_impl("):
        names |= _reads(_body(capi, head))
    return names


def _test_text(name):
    with open(os.path.join(TESTS, name)) as f:
        return f.read()


def test_every_environment_read_has_exactly_one_row():
    src = _sources()
    read = set().union(*(_reads(t) for t in src.values()))
    table = set(knob_table.KNOBS)
    assert not read - table, "knobs the library reads but tests/knob_table.py does not list: %s" % sorted(read - table)
    assert not table - read, "rows of tests/knob_table.py for knobs the library no longer reads: %s" % sorted(table - read)


def test_the_scanner_skips_macros_codes_and_comments():
    src = _sources()
    read = set().union(*(_reads(t) for t in src.values()))
    everything = "\n".join(src.values())
    for name in ("UGP_HOT_SLOTS", "UGP_FS_B", "UGP_OK", "UGP_ERR_UNSUPPORTED"):   # compile-time macros and return codes
        assert re.search(r"\b%s\b" % name, everything), name
        assert name not in read, name
    assert _reads(_strip_comments('x = 1;   // getenv("UGP_IN_A_COMMENT")\n/* flag("UGP_IN_A_BLOCK") */')) == set()
    assert _reads(_strip_comments('const char *e = getenv("UGP_A"); k.b = num("UGP_B", 2); k.c = pos( "UGP_C");')) == {"UGP_A", "UGP_B", "UGP_C"}


def test_rows_are_well_formed():
    for name, row in knob_table.KNOBS.items():
        assert isinstance(row, tuple) and len(row) == 2, name
        cls, why = row
        assert cls in ("grid", "diagnostic") or cls.startswith("tested:"), (name, cls)
        assert isinstance(why, str) and why.strip(), name
    for name, why in knob_table.FLATTEN.items():
        assert name in knob_table.KNOBS, name
        assert isinstance(why, str) and why.strip(), name


def test_tested_rows_name_a_test_file_that_uses_the_knob():
    for name, (cls, _) in knob_table.KNOBS.items():
        if cls.startswith("tested:"):
            f = cls[len("tested:"):]
            assert f.startswith("test_") and f.endswith(".py") and f != GRID_FILE, (name, f)
            assert os.path.isfile(os.path.join(TESTS, f)), (name, f)
            assert re.search(r"\b%s\b" % name, _test_text(f)), "%s: %s does not name it" % (name, f)


def test_grid_rows_are_in_the_gpu_grid():
    text = _test_text(GRID_FILE)
    for name, (cls, _) in knob_table.KNOBS.items():
        if cls == "grid":
            assert re.search(r"\b%s\b" % name, text), "%s: %s does not name it" % (name, GRID_FILE)


def test_flattening_knobs_are_in_the_signature_or_say_why_not():
    src = _sources()
    sig = _signature_names(src["ugp_capi.cpp"])
    flat = _flatten_reads(src)
    assert not flat - set(knob_table.FLATTEN), "knobs read while flattening without a FLATTEN row: %s" % sorted(flat - set(knob_table.FLATTEN))
    for name, why in knob_table.FLATTEN.items():
        if why == "signature":
            assert name in sig, "%s is marked as hashed by flat_signature(), which does not list it" % name
        else:
            assert name not in sig, "%s is in flat_signature(): mark its FLATTEN row \"signature\"" % name
    assert not sig - set(knob_table.FLATTEN), sorted(sig - set(knob_table.FLATTEN))
    assert not sig - set(knob_table.KNOBS), sorted(sig - set(knob_table.KNOBS))


def test_the_knob_header_points_at_the_table_and_this_test():
    with open(os.path.join(CSRC, "ugp_knobs.hpp")) as f:
        head = f.read().split("#pragma once")[0]
    assert "tests/knob_table.py" in head and "tests/test_knob_inventory.py" in head
