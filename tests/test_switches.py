"""docs/SWITCHES.md against the code: every HIFIHR_* environment variable the package reads has a row in the table, every row names a
variable that is read, and every row's "used by" is true.  A switch survives only while a test, bench.py, tools/ablation.sh or an operator
of a training run uses it (the A/B levers of decided experiments are retired: docs/HISTORY.md); a new one has to be justified in the
table or this test fails; every value tools/ablation.sh times has an arm with parity cases in tests/switch_arms.py.  Text only: no library
is loaded."""
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


def _ablation_assignments():
    """[{variable: value}] of the rows of tools/ablation.sh that set a variable"""
    rows = []
    for line in _text(os.path.join(ROOT, "tools", "ablation.sh")).splitlines():
        if line.startswith("run "):
            env = dict(re.findall(r"\s(HIFIHR_[A-Z0-9_]+)=(\S+)", line.split('"', 2)[2]))
            if env:
                rows.append(env)
    return rows


def test_every_ablation_value_has_an_arm_with_parity_cases():
    """A timing of an arm that computes something else is worth nothing, and an A/B lever must not arrive without parity for its other arm:
    every variable assignment of tools/ablation.sh, and every row of docs/SWITCHES.md that names `ablation`, is the environment of an arm
    of tests/switch_arms.py (exactly that value), which has cases and a witness -- or says why a device cannot see it -- on every device
    it runs on.  (tests/test_hostsim_switch_arms.py and tests/test_gpu_switch_arms.py run the arms.)"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import switch_arms as sa
    envs = [a["env"] for n, a in sa.ARMS.items() if n != "default"]
    rows = _ablation_assignments()
    assert len(rows) > 25, "the scan found the rows of tools/ablation.sh"
    for env in rows:
        assert env in envs, f"tools/ablation.sh times {env}: no arm of tests/switch_arms.py has exactly this environment"
    timed = {k for env in rows for k in env}
    for name, users in sorted(_table().items()):
        if "ablation" in users:
            assert name in timed, f"{name}: docs/SWITCHES.md says tools/ablation.sh uses it, and no row there sets it"
            assert any(set(env) == {name} for env in envs), f"{name}: no arm of tests/switch_arms.py for this switch alone"
            assert "test" in users, f"{name}: its arm is tested; say so in its 'Used by' cell"
    for env in envs:              # (an arm beyond the script's rows is a value the table documents: HIFIHR_CONV_ROWS=2)
        assert set(env) <= set(_table()), f"tests/switch_arms.py has an arm {env} of a variable without a row in docs/SWITCHES.md"
    for n, a in sa.ARMS.items():
        for device in sa.devices(a):
            assert sa.cases(a, device), f"{n}: no cases on {device}"
            assert n == "default" or sa.witness(a, device) or a["unseen"].get(device), f"{n}: neither a witness nor a reason on {device}"
