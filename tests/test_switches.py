"""docs/SWITCHES.md against the code: every HIFIHR_* environment variable the package reads has a row in the table, every row names a
variable that is read, and every row's "used by" is true.  A switch survives only while a test, bench.py, tools/ablation.sh or an operator
of a training run uses it (the A/B levers of decided experiments are retired: docs/HISTORY.md); a new one has to be justified in the
table or this test fails.  Text only: no library is loaded."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READ = re.compile(r'(?:getenv|env_int|environ(?:\.get)?)[\(\[]"(HIFIHR_[A-Z0-9_]+)"')
NAME = re.compile(r"\bHIFIHR_[A-Z0-9_]+\b")
OPERATOR = {"HIFIHR_DIST_BACKEND", "HIFIHR_DIST_TIMEOUT_MIN", "HIFIHR_DP_TRACE", "HIFIHR_DEBUG_SYNC"}
USERS = ("test", "bench", "ablation", "operator")


def _text(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _walk(top):
    for d, dirs, files in os.walk(top):
        dirs[:] = [x for x in dirs if x not in ("__pycache__", "build", "build_asan")]
        for n in files:
            if not n.endswith((".so", ".o", ".pyc", ".npz", ".npy", ".png", ".bin", ".pt")):
                yield os.path.join(d, n)


def _names_read():
    found = set()
    for path in list(_walk(os.path.join(ROOT, "hifihr_amd"))) + [os.path.join(ROOT, "train_hrnet.py")]:
        found.update(READ.findall(_text(path)))
    return found


def _table():
    """{switch: set of users} from the rows of docs/SWITCHES.md (first cell: the name in backticks, last cell: the users)."""
    rows = {}
    for line in _text(os.path.join(ROOT, "docs", "SWITCHES.md")).splitlines():
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        m = re.fullmatch(r"`(HIFIHR_[A-Z0-9_]+)`", cells[0]) if line.startswith("|") else None
        if m:
            assert m.group(1) not in rows, f"{m.group(1)}: two rows"
            assert len(cells) == 6, f"{m.group(1)}: a row has six cells"
            rows[m.group(1)] = {u.strip() for u in cells[-1].split(",")}
    return rows


def _named_by():
    me = os.path.abspath(__file__)
    tests = set()
    for path in _walk(os.path.join(ROOT, "tests")):
        if os.path.abspath(path) != me:
            tests.update(NAME.findall(_text(path)))
    return {"test": tests, "bench": set(NAME.findall(_text(os.path.join(ROOT, "bench.py")))),
            "ablation": set(NAME.findall(_text(os.path.join(ROOT, "tools", "ablation.sh")))), "operator": OPERATOR}


def test_every_switch_read_is_in_the_table_and_every_row_is_read():
    read, rows = _names_read(), _table()
    assert len(read) > 30, "the scan found the package's reads"
    assert read - set(rows) == set(), "read in the code without a row in docs/SWITCHES.md (justify it there, or retire it)"
    assert set(rows) - read == set(), "rows of docs/SWITCHES.md that nothing reads any more"


def test_every_row_names_its_users_truthfully():
    named = _named_by()
    for name, users in sorted(_table().items()):
        assert users and users <= set(USERS), f"{name}: 'used by' is a list of {USERS}, got {sorted(users)}"
        for u in users:
            assert name in named[u], f"{name}: the table says '{u}' uses it, and it does not"


def test_every_switch_has_a_user():
    named = _named_by()
    for name in sorted(_names_read()):
        assert any(name in named[u] for u in USERS), f"{name}: named by no test, not by bench.py, tools/ablation.sh or the operator list"
