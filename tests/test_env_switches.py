"""The environment variables the product reads are exactly the documented ones: every name the
library sources pass to getenv() and the package passes to os.environ / os.getenv(), against the
first column of INTEGRATION.md's "Environment variables" table.  A new switch cannot enter
undocumented, and a documented one cannot silently disappear."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "indy-plenum_amd")

_C_GETENV = re.compile(r'\bgetenv\(\s*"([^"]+)"')
_PY_ENV = re.compile(r'\bos\.(?:environ\.get\(|environ\[|getenv\()\s*["\']([^"\']+)["\']')


def _names(paths, pattern):
    assert paths
    found = set()
    for path in paths:
        with open(path, encoding="utf-8") as f:
            found.update(pattern.findall(f.read()))
    return found


def _read_by_the_sources():
    c_files = [p for ext in ("h", "hip", "cpp") for p in glob.glob(os.path.join(PKG, "csrc", "*." + ext))]
    py_files = glob.glob(os.path.join(PKG, "plenum_amd", "*.py"))
    return _names(c_files, _C_GETENV) | _names(py_files, _PY_ENV)


def _documented():
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as f:
        text = f.read()
    section = re.search(r"^## [^\n]*Environment variables\n(.*?)(?=^## |\Z)", text, re.M | re.S)
    assert section, 'INTEGRATION.md has no "Environment variables" section'
    rows = [line for line in section.group(1).splitlines() if line.startswith("|")]
    assert len(rows) > 2 and set(rows[1]) <= set("|-: "), "one table: a header, a rule, then rows"
    names = [re.fullmatch(r"`(\w+)`", row.split("|")[1].strip()) for row in rows[2:]]
    assert all(names), "the first column holds one back-quoted name per row"
    names = [m.group(1) for m in names]
    assert len(names) == len(set(names)), "a name is documented twice"
    return set(names)


def test_the_patterns_find_every_spelling():
    c = 'x = getenv("A_B"); if (std::getenv( "C")) y = mygetenv("D");'
    assert _C_GETENV.findall(c) == ["A_B", "C"]
    py = 'a = os.environ.get("P", "1"); b = os.environ["Q"]; c = os.getenv(\'R\'); d = cosmos.getenv("S")'
    assert _PY_ENV.findall(py) == ["P", "Q", "R"]


def test_every_environment_variable_read_is_documented_and_every_documented_one_is_read():
    read, documented = _read_by_the_sources(), _documented()
    assert read - documented == set(), "read by the sources but missing from INTEGRATION.md's table"
    assert documented - read == set(), "in INTEGRATION.md's table but read nowhere"
    assert read == documented
