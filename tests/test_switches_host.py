"""The library's environment switches (csrc/switches.h), checked on the host.

tests/host/switches_check.cpp includes only that header; it is built with AddressSanitizer + UndefinedBehaviorSanitizer and run once
per mode in a fresh process (a Once row keeps its first read for the life of a process): unset -> off, "1" -> on, "0" -> on iff Any,
a PerCall row follows a later change and a Once row does not, switch_text returns the text or null.

The text checks read files only.  They keep the table the one place that names a switch: no getenv and no quoted NGPDE_ name in
csrc outside the header, DESIGN.md section 5.8 lists the header's rows, its second list is what the package reads itself, and every
switch a test drives is in one of the two lists (a test left driving a switch that no longer exists would pass without reaching
anything).
"""
import glob
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "neuralgraphpde.jl_amd")
CSRC = os.path.join(PKG, "csrc")
HEADER = os.path.join(CSRC, "switches.h")
MODES = ("unset", "one", "zero", "text")
ROW = re.compile(r'^\s*X\((\w+),\s*"(NGPDE_[A-Z0-9_]+)",\s*(Once|PerCall),\s*(Any|One|Text),\s*"([^"]+)"\)\s*\\?$', re.M)
# variables of the benchmark and of the suite's own conftest, not switches of the library or the package
NOT_SWITCHES = ("NGPDE_BENCH_", "NGPDE_TEST_")


def read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def header_rows():
    text = read(HEADER)
    rows = ROW.findall(text)
    assert len(rows) == len(re.findall(r"^\s*X\(", text, re.M)), "a row of the table is not in the regular one-line format"
    return rows


def design_lists():
    """(names of section 5.8's table, names of its list of package-side switches)"""
    text = read(os.path.join(ROOT, "DESIGN.md"))
    sec = text[text.index("### 5.8 "):text.index("### 5.9 ")]
    table = re.findall(r"^\| `(NGPDE_[A-Z0-9_]+)` \| (Once|PerCall) \| (Any|One|Text) \|", sec, re.M)
    listed = re.findall(r"^- `(NGPDE_[A-Z0-9_]+)`", sec, re.M)
    return table, listed


@pytest.fixture(scope="module")
def check_program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("switches") / "switches_check")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-g", "-O1", "-I", CSRC, os.path.join(HERE, "host", "switches_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("mode", MODES)
def test_every_row_follows_its_read_time_and_meaning_of_on(check_program, mode):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([check_program, mode], capture_output=True, text=True, timeout=60, env=env)
    report = r.stdout + r.stderr
    assert r.returncode == 0, report[-3000:]
    assert "AddressSanitizer" not in report and "runtime error" not in report and "LeakSanitizer" not in report, report[-3000:]
    assert f"{len(header_rows())} rows, 0 failed checks" in r.stdout


def test_the_table_is_regular_and_names_each_switch_once():
    rows = header_rows()
    assert len(rows) >= 30
    assert len({r[0] for r in rows}) == len(rows) and len({r[1] for r in rows}) == len(rows)


def test_no_getenv_in_csrc_outside_the_header():
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.isfile(path) and path != HEADER and path.endswith((".hip", ".h", ".cpp", ".c")):
            assert "getenv" not in read(path), os.path.basename(path)


def test_no_quoted_switch_name_in_the_hip_files():
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        assert re.search(r'"NGPDE_', read(path)) is None, os.path.basename(path)


def test_design_table_lists_the_headers_rows():
    table, _ = design_lists()
    assert sorted(table) == sorted((name, rd, on) for _, name, rd, on, _ in header_rows())


def test_design_second_list_is_what_the_package_reads_itself():
    _, listed = design_lists()
    assert listed
    src = "".join(read(p) for p in sorted(glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True)))
    looked_up = set(re.findall(r'os\.environ(?:\.get\(|\[)\s*"(NGPDE_[A-Z0-9_]+)"', src))
    assert set(listed) == looked_up


def test_every_switch_a_test_drives_is_listed():
    table, listed = design_lists()
    known = {name for name, _, _ in table} | set(listed)
    for path in sorted(glob.glob(os.path.join(HERE, "*.py"))):
        # a whole quoted name: monkeypatch.setenv / delenv, os.environ lookups, and the tuples of names the tests loop over
        for name in re.findall(r'"(NGPDE_[A-Z0-9_]+)"', read(path)):
            if not name.startswith(NOT_SWITCHES):
                assert name in known, f"{os.path.basename(path)} drives {name}, which neither list of DESIGN.md section 5.8 has"
