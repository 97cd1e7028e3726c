"""The one place that starts, gates, releases, waits for and reaps the helper processes of the GPU tests.

A helper is registered with spawn() -- by its module's start_children(), which tests/conftest.py calls once the collection holds a
test of that module and before the session touches the GPU -- and collected with result().  What is started at spawn() is only
tests/gated_run.py, which opens no GPU: it waits on its stdin, the gate, until the helper is released, and then runs the command under
the helper's own time limit.

Release.  The shared GPU boxes allow 16 processes with the GPU open at once.  One is the session; one is left for whatever a
developer or a nested run has open beside it; two are spare: BUDGET = 16 - 1 - 1 - 2 = 12 processes beside the session.  Every helper
states how many processes it will open the GPU from (`gpu_procs`: the ranks of a torch.distributed.run child, 1 for a worker or a nested
pytest child).  Helpers are released in the order they were registered -- the same on every run -- as long as the released and
unfinished ones stay within the budget; one that a test is waiting for in result() goes to the front of those still gated.  One
pump does it, called from spawn() and result(); there are no threads: a waiting result() polls the running helpers a few times per
second.

Stop.  After a GPU fault or hang nothing more is started on the GPU: once a helper ends with 124 (its time limit), 134 (abort), 137
(killed) or 139 (segmentation fault) no further helper is released, and result() of one still waiting fails, naming the one that
died and its log.  An ordinary non-zero exit stops nothing.  No helper is ever started twice.

At exit every live process group is ended, and the release / finish timeline (name, gpu_procs, times, status) goes to children.json
beside the parity_measured.json that tests/conftest.py writes at the end of the session."""
import atexit
import collections
import glob
import json
import os
import signal
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_F16 = os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so")
BUDGET = 12
DEAD = (124, 134, 137, 139)
POLL_S = 0.25
TIMELINE = None         # a path of the caller's; None: children.json beside the session's parity_measured.json

Result = collections.namedtuple("Result", "rc log")

_KIDS = {}              # name -> record, in registration order
_T0 = time.time()


def tmpdir(name):
    """The helper's own temporary directory (its log lives there; the caller may put the helper's output beside it)."""
    if name not in _KIDS:
        _KIDS[name] = {"name": name, "tmp": tempfile.mkdtemp(prefix=f"octmae_{name}_"), "proc": None}
    return _KIDS[name]["tmp"]


def spawn(name, cmd, env=None, gpu_procs=1, limit_s=300, stdout=None):
    """Registers the helper `name` and starts its launcher, gate closed (idempotent per name).  `stdout`: a file for the command's
    standard output where a test reads it apart from the log."""
    assert gpu_procs <= BUDGET, f"{name}: {gpu_procs} GPU processes exceed the budget of {BUDGET}"
    tmpdir(name)
    if _KIDS[name]["proc"]:
        return
    if not any(k["proc"] for k in _KIDS.values()):
        atexit.register(_at_exit)
    k = _KIDS[name] = _KIDS.pop(name)                  # registration order is the order of the spawn() calls
    k["log"] = os.path.join(k["tmp"], "child.log")
    launcher = [sys.executable, os.path.join(ROOT, "tests", "gated_run.py"), "--limit", str(limit_s)] + (["--stdout", stdout] if stdout else [])
    with open(k["log"], "wb") as logf:                 # a file, not a pipe: a chatty helper never blocks on a full pipe
        proc = subprocess.Popen(launcher + ["--", *cmd], cwd=ROOT, env=env, stdin=subprocess.PIPE, stdout=logf, stderr=subprocess.STDOUT,
                                start_new_session=True)
    k.update(proc=proc, gpu_procs=gpu_procs, limit_s=limit_s, registered=time.time(), wanted=False, released=None, finished=None, rc=None)
    _pump()


def _died():
    return next((k for k in _KIDS.values() if k["proc"] and k["rc"] in DEAD), None)


def _pump():
    """Notes the helpers that have ended, then releases the next ones in registration order while the budget holds."""
    kids = [k for k in _KIDS.values() if k["proc"]]
    for k in kids:
        if k["released"] is not None and k["rc"] is None and k["proc"].poll() is not None:
            k.update(rc=k["proc"].returncode, finished=time.time())
    if _died():
        return
    used = sum(k["gpu_procs"] for k in kids if k["released"] is not None and k["rc"] is None)
    for k in sorted(kids, key=lambda k: not k["wanted"]):     # stable: registration order among the wanted, then among the rest
        if k["released"] is None:
            if used + k["gpu_procs"] > BUDGET:
                break
            used += k["gpu_procs"]
            k["released"] = time.time()
            try:
                k["proc"].stdin.write(b"go\n")
                k["proc"].stdin.close()
            except OSError:                            # the launcher is gone: its status says why
                pass


def result(name):
    """Releases the helper if that has not happened yet, waits for it, and returns (return code, log path); the same record on every
    later call."""
    k = _KIDS[name]
    assert k["proc"], f"{name} was never spawned"
    k["wanted"] = True
    while k["rc"] is None:
        _pump()
        if k["rc"] is None:
            d = _died()
            assert k["released"] is not None or d is None, \
                f"{name} was not started: {d['name']} ended with status {d['rc']} before it and nothing more runs on the GPU; its log: {d['log']}"
            time.sleep(POLL_S)
    return Result(k["rc"], k["log"])


def log_tail(name, n=3000):
    with open(_KIDS[name]["log"], "rb") as f:
        text = f.read().decode(errors="replace")
    return text if n is None else text[-n:]


def spawn_f16_worker(name, call, limit_s=300, ext="json"):
    """tests/f16_worker.py --call `call` on the half-operand build (a process binds one library: octcubem_amd/_lib.py)."""
    out = _KIDS[name]["out"] = os.path.join(tmpdir(name), "result." + ext)
    spawn(name, [sys.executable, os.path.join(ROOT, "tests", "f16_worker.py"), "--call", call, "--out", out],
          env=dict(os.environ, OCTMAE_LIB=LIB_F16), limit_s=limit_s)


def f16_worker_result(name):
    """What the worker wrote: the dict of a JSON result, the NpzFile of an npz one."""
    rc, out = result(name).rc, _KIDS[name]["out"]
    assert rc == 0 and os.path.exists(out), f"rc {rc}\n{log_tail(name)}"
    if out.endswith(".json"):
        with open(out) as f:
            return json.load(f)
    import numpy as np
    return np.load(out)


def _end_all():
    """SIGTERM to every live launcher, which ends its command's process group (tests/gated_run.py); SIGKILL to what is left."""
    live = [k for k in _KIDS.values() if k["proc"] and k["proc"].poll() is None]
    for sig in (signal.SIGTERM, signal.SIGKILL):
        for k in live:
            if k["proc"].poll() is None:
                try:
                    os.killpg(k["proc"].pid, sig)
                except ProcessLookupError:
                    pass
        t_end = time.time() + 15
        while sig == signal.SIGTERM and any(k["proc"].poll() is None for k in live) and time.time() < t_end:
            time.sleep(0.05)
    for k in live:
        k["proc"].wait()
        if k["proc"].stdin and not k["proc"].stdin.closed:
            k["proc"].stdin.close()


def timeline():
    rel = lambda t: None if t is None else round(t - _T0, 3)  # noqa: E731
    return [{"name": k["name"], "gpu_procs": k["gpu_procs"], "limit_s": k["limit_s"], "registered": rel(k["registered"]),
             "released": rel(k["released"]), "finished": rel(k["finished"]), "status": k["rc"]} for k in _KIDS.values() if k["proc"]]


def _at_exit():
    _end_all()
    try:
        ledgers = glob.glob(os.path.join(ROOT, "*", "parity_measured.json"))        # tests/conftest.py::_parity_ledger
        path = TIMELINE or os.path.join(os.path.dirname(max(ledgers, key=os.path.getmtime)), "children.json")
        with open(path, "w") as f:
            json.dump(timeline(), f, indent=1)
    except (OSError, ValueError):                      # no ledger of a session to lie beside, or no room: no timeline
        pass
