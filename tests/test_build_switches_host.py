"""The table "Build-time switches" of tools/README.md against the sources (text only, no GPU, nothing compiled):

* every ``#ifndef NAME`` / ``#define NAME value`` pair of noisereduce_amd/csrc/*.hpp and *.hip has a row, in the file the row
  names and with the default the row states;
* every row names a macro that the file it names still tests or defines.

A switch that is added, renamed or deleted without its row fails here; so does a row left behind."""
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "noisereduce_amd", "csrc")


def _sources():
    return {os.path.basename(p): open(p).read()
            for ext in ("*.hpp", "*.hip") for p in sorted(glob.glob(os.path.join(CSRC, ext)))}


def _pairs():
    """[(file, NAME, default)]: an #ifndef whose next line defines the same name."""
    out = []
    for name, text in _sources().items():
        for m in re.finditer(r"^[ \t]*#[ \t]*ifndef[ \t]+(\w+)[^\n]*\n[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]*([^\s/]*)", text, re.M):
            if m.group(1) == m.group(2):
                out.append((name, m.group(1), m.group(3)))
    return out


def _table():
    """{NAME: (default, [files])} of the README's table."""
    text = open(os.path.join(ROOT, "tools", "README.md")).read()
    body = text.split("## Build-time switches", 1)[1]
    rows = {}
    for ln in body.splitlines():
        m = re.match(r"\| `(\w+)` \| ([^|]+) \| ([^|]+) \|", ln)
        if m:
            assert m.group(1) not in rows, "two rows for " + m.group(1)
            rows[m.group(1)] = (m.group(2).strip(), re.findall(r"`([\w.]+)`", m.group(3)))
    return rows


PAIRS = _pairs()
TABLE = _table()


def test_there_is_something_to_check():
    assert len(PAIRS) >= 10 and len(TABLE) >= len({n for _, n, _ in PAIRS})
    assert ("onepass.hpp", "OP_TRACE", "0") in PAIRS and ("api.hip", "SG_TEAM_N", "2048") in PAIRS


@pytest.mark.parametrize("src,name,default", PAIRS, ids=["%s:%s" % (s, n) for s, n, _ in PAIRS])
def test_every_switch_has_its_row(src, name, default):
    assert name in TABLE, "%s (%s) has no row in tools/README.md, 'Build-time switches'" % (name, src)
    row_default, files = TABLE[name]
    assert src in files, "%s: the row names %s, the switch is in %s" % (name, files, src)
    assert row_default == default, "%s: default %s in %s, %s in the table" % (name, default, src, row_default)


def test_a_switch_has_one_default():
    names = [n for _, n, _ in PAIRS]
    assert len(names) == len(set(names)), sorted(n for n in set(names) if names.count(n) > 1)


@pytest.mark.parametrize("name", sorted(TABLE))
def test_every_row_names_a_macro_that_exists(name):
    src = _sources()
    _, files = TABLE[name]
    assert files, name
    for f in files:
        assert f in src, "%s: no such file %s" % (name, f)
        assert re.search(r"^[ \t]*#[ \t]*(if|ifdef|ifndef|elif|define)\b[^\n]*\b%s\b" % name, src[f], re.M), \
            "%s is not tested or defined by a preprocessor line of %s" % (name, f)
