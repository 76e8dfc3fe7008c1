"""The environment table of INTEGRATION.md lists exactly the MOGP_* variables the library reads: the names passed to getenv in mogptk_amd/csrc
and those read from os.environ in the Python package.  A switch added or retired without its row fails here."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def names_read_by_the_code():
    names = set()
    csrc = os.path.join(ROOT, "mogptk_amd", "csrc")
    for path in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")):
        names |= set(re.findall(r'getenv\(\s*"(MOGP_[A-Z0-9_]+)"', _read(path)))
    for path in glob.glob(os.path.join(ROOT, "mogptk_amd", "**", "*.py"), recursive=True):
        names |= set(re.findall(r'environ(?:\.get\(|\[|\.setdefault\(|\.pop\()\s*["\'](MOGP_[A-Z0-9_]+)["\']', _read(path)))
        names |= set(re.findall(r'getenv\(\s*["\'](MOGP_[A-Z0-9_]+)["\']', _read(path)))
    return names


def names_in_the_table():
    text = _read(os.path.join(ROOT, "INTEGRATION.md"))
    section = text.split("## Environment switches", 1)[1].split("\n## ", 1)[0]
    rows = [l for l in section.split("\n") if l.startswith("| `MOGP_")]
    names = set()
    for row in rows:
        first = re.split(r"(?<!\\)\|", row)[1]                 # the variables of a row stand in its first column (\| inside a cell is no border)
        names |= set(re.findall(r"MOGP_[A-Z0-9_]+", first))
    return names


def test_the_environment_table_lists_exactly_the_variables_the_library_reads():
    code, table = names_read_by_the_code(), names_in_the_table()
    assert len(code) >= 20, sorted(code)                       # the scan found the sources
    assert code == table, "read but not in INTEGRATION.md: %s; in INTEGRATION.md but not read: %s" % (sorted(code - table), sorted(table - code))


def test_the_k_range_shortening_switch_is_gone():
    assert "MOGP_FAKE_K" not in names_read_by_the_code()
    assert "MOGP_FAKE_K" not in names_in_the_table()
