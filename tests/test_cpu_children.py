"""tests/children.py and tests/gated_run.py, without a GPU: the helpers here are `python -c` one-liners that touch marker files, sleep
or sys.exit(n) -- no torch, no package, no real fault.  Every test works on a private copy of the module, so the helpers of a GPU
session that runs beside these tests, and its timeline, are left alone."""
import atexit
import importlib.util
import json
import os
import signal
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATED_RUN = os.path.join(ROOT, "tests", "gated_run.py")


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture
def ch(tmp_path):
    mod = _load(os.path.join(ROOT, "tests", "children.py"), "children_under_test")
    mod.TIMELINE = str(tmp_path / "children.json")
    yield mod
    mod._end_all()
    atexit.unregister(mod._at_exit)


def py(code):
    return [sys.executable, "-c", code]


def touch(path):
    return py(f"open({str(path)!r}, 'a').write('x\\n')")


def alive(pid):
    try:
        with open(f"/proc/{pid}/stat") as f:
            return f.read().rsplit(")", 1)[1].split()[0] != "Z"
    except OSError:
        return False


def wait_for(path, seconds=10.0):
    t_end = time.time() + seconds
    while not os.path.exists(path) or not open(path).read().strip():
        assert time.time() < t_end, f"{path} never appeared"
        time.sleep(0.05)
    return open(path).read().split()


def test_an_unreleased_child_has_not_run(ch, tmp_path):
    ch.spawn("blocker", py("import time; time.sleep(1.0)"), gpu_procs=ch.BUDGET)
    ch.spawn("waiting", touch(tmp_path / "ran"))
    time.sleep(0.5)
    assert not (tmp_path / "ran").exists()
    assert [k["released"] is not None for k in ch.timeline()] == [True, False]
    assert ch.result("waiting").rc == 0 and (tmp_path / "ran").exists()
    assert ch.result("blocker").rc == 0


def test_a_child_a_test_waits_for_goes_before_the_other_gated_ones(ch, tmp_path):
    ch.spawn("blocker", py("import time; time.sleep(0.5)"), gpu_procs=ch.BUDGET)
    ch.spawn("first", touch(tmp_path / "first"), gpu_procs=ch.BUDGET)
    ch.spawn("asked", touch(tmp_path / "asked"), gpu_procs=ch.BUDGET)
    assert ch.result("asked").rc == 0 and not (tmp_path / "first").exists()
    assert ch.result("first").rc == 0
    assert [k["name"] for k in sorted(ch.timeline(), key=lambda k: k["released"])] == ["blocker", "asked", "first"]


def test_spawn_is_idempotent_and_result_is_cached(ch, tmp_path):
    for _ in range(2):
        ch.spawn("once", touch(tmp_path / "runs"))
    first = ch.result("once")
    ch.spawn("once", touch(tmp_path / "runs"))
    assert ch.result("once") == first and first.rc == 0 and os.path.exists(first.log)
    assert (tmp_path / "runs").read_text() == "x\n"
    assert [k["name"] for k in ch.timeline()] == ["once"]
    with pytest.raises(AssertionError):
        ch.spawn("too wide", touch(tmp_path / "never"), gpu_procs=ch.BUDGET + 1)


def test_todays_mix_stays_within_the_budget_by_its_own_timeline(ch):
    """The weights of today's GPU session on a two-GPU box: tests/test_gpu_comm.py's ranks (2 + 4 + 2 + 2), the two parity ledgers, the
    nested kernel suite, then eight workers."""
    weights = [10, 1, 1, 1] + [1] * 8
    for i, w in enumerate(weights):
        ch.spawn(f"c{i:02d}", py(f"import time; time.sleep({0.3 + 0.1 * (i % 3)})"), gpu_procs=w)
    assert all(ch.result(f"c{i:02d}").rc == 0 for i in range(len(weights)))
    line = ch.timeline()
    assert [k["name"] for k in line] == [f"c{i:02d}" for i in range(len(weights))] and [k["gpu_procs"] for k in line] == weights
    assert all(k["released"] is not None and k["finished"] >= k["released"] for k in line)
    assert [k["released"] for k in line] == sorted(k["released"] for k in line)           # registration order
    peak = max(sum(o["gpu_procs"] for o in line if o["released"] <= k["released"] < o["finished"]) for k in line)
    assert peak == ch.BUDGET == 12, peak            # 10 + 1 + 1 at once; the fourth waits for room


def test_the_limit_gives_124_and_leaves_nothing_of_the_group_alive(ch, tmp_path):
    pids = tmp_path / "pids"
    code = ("import os, subprocess, sys, time; g = subprocess.Popen([sys.executable, '-c', 'import time; time.sleep(60)']); "
            f"open({str(pids)!r}, 'w').write(f'{{os.getpid()}} {{g.pid}}'); time.sleep(60)")
    ch.spawn("sleeper", py(code), limit_s=2)
    t0 = time.time()
    assert ch.result("sleeper").rc == 124
    assert time.time() - t0 < 8.0
    child, grandchild = (int(p) for p in pids.read_text().split())
    assert not alive(child) and not alive(grandchild)


def test_after_a_fault_status_nothing_more_is_released(ch, tmp_path):
    ch.spawn("crashed", py("import sys; sys.exit(139)"), gpu_procs=ch.BUDGET)
    ch.spawn("next", touch(tmp_path / "ran"))
    assert ch.result("crashed").rc == 139
    with pytest.raises(AssertionError) as e:
        ch.result("next")
    assert "crashed" in str(e.value) and "139" in str(e.value) and ch.result("crashed").log in str(e.value)
    ch.spawn("later", touch(tmp_path / "ran"))
    with pytest.raises(AssertionError):
        ch.result("later")
    assert not (tmp_path / "ran").exists()
    assert [k["released"] is not None for k in ch.timeline()] == [True, False, False]


def test_an_ordinary_failure_stops_nothing(ch, tmp_path):
    ch.spawn("failed", py("import sys; sys.exit(1)"), gpu_procs=ch.BUDGET)
    ch.spawn("next", touch(tmp_path / "ran"))
    assert ch.result("failed").rc == 1
    assert ch.result("next").rc == 0 and (tmp_path / "ran").exists()


def test_the_reaper_ends_a_live_group_and_writes_the_timeline(ch, tmp_path):
    pid = tmp_path / "pid"
    ch.spawn("running", py(f"import os, time; open({str(pid)!r}, 'w').write(str(os.getpid())); time.sleep(60)"))
    ch.spawn("gated", touch(tmp_path / "ran"), gpu_procs=ch.BUDGET)
    running = int(wait_for(pid)[0])
    assert alive(running)
    ch._at_exit()
    assert not alive(running) and not (tmp_path / "ran").exists()
    assert all(k["proc"].poll() is not None for k in ch._KIDS.values())
    line = json.load(open(ch.TIMELINE))
    assert [(k["name"], k["gpu_procs"], k["released"] is not None, k["status"]) for k in line] == [("running", 1, True, None), ("gated", 12, False, None)]


def test_the_launcher_exits_2_on_eof_and_passes_the_childs_status_on(tmp_path):
    launch = [sys.executable, GATED_RUN, "--limit", "5", "--"]
    r = subprocess.run(launch + touch(tmp_path / "ran"), stdin=subprocess.DEVNULL, timeout=30)
    assert r.returncode == 2 and not (tmp_path / "ran").exists()
    r = subprocess.run(launch + py("import sys; sys.exit(7)"), input=b"go\n", timeout=30)
    assert r.returncode == 7
    out = tmp_path / "stdout"                       # a death by signal n is 128 + n; --stdout keeps the standard output apart
    r = subprocess.run(launch[:-1] + ["--stdout", str(out), "--"] + py("import os, signal; print('line', flush=True); os.kill(os.getpid(), signal.SIGUSR1)"),
                       input=b"go\n", timeout=30)
    assert r.returncode == 128 + signal.SIGUSR1 and out.read_text() == "line\n"


def test_importing_the_comm_tests_starts_no_process(monkeypatch):
    """`--collect-only` and `-m "not gpu"` import tests/test_gpu_comm.py but never call its start_children() (tests/conftest.py calls it
    only for a module with a selected test): with GPUs visible the import alone must start nothing."""
    import torch
    from tests import children
    started = []
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 2)
    monkeypatch.setattr(subprocess, "Popen", lambda *a, **k: started.append(a) or pytest.fail("a process was started at import"))
    before = list(children._KIDS)
    mod = _load(os.path.join(ROOT, "tests", "test_gpu_comm.py"), "test_gpu_comm_under_test")
    assert not started and list(children._KIDS) == before
    assert callable(mod.start_children) and mod.TWO_GPUS and mod.ONE_GPU
