"""python tests/gated_run.py --limit S [--stdout PATH] -- CMD...

The launcher tests/children.py puts in front of every GPU helper process.  It imports neither torch nor the package, so it never opens
the GPU itself.  It reads one line from stdin -- the gate -- and exits 2 when stdin ends without one (the session went away without
asking).  Then it runs CMD as a child process in a process group of its own (it does not exec it), waits at most S seconds, and

  * on the limit ends the child's process group and exits 124;
  * otherwise exits with the child's status, a death by signal n as 128 + n.

A SIGTERM to the launcher (the session's reaper) ends the child's group as well.  "Ends a group": SIGTERM, so that a
torch.distributed.run child takes its ranks with it (each rank is a session of its own), a few seconds of grace, then SIGKILL.
--stdout keeps CMD's standard output in a file of its own for the tests that read it apart from the log."""
import os
import signal
import subprocess
import sys
import time

GRACE_S = 5.0


def end_group(child):
    for sig in (signal.SIGTERM, signal.SIGKILL):
        try:
            os.killpg(child.pid, sig)
        except ProcessLookupError:
            pass
        t_end = time.monotonic() + GRACE_S
        while sig == signal.SIGTERM and child.poll() is None and time.monotonic() < t_end:
            time.sleep(0.05)
    child.wait()


def main(argv):
    opts, cmd = argv[:argv.index("--")], argv[argv.index("--") + 1:]
    limit_s = float(opts[opts.index("--limit") + 1])
    stdout = open(opts[opts.index("--stdout") + 1], "wb") if "--stdout" in opts else None
    if not sys.stdin.readline():
        return 2
    child = []

    def on_term(signum, frame):
        if child:
            end_group(child[0])
        sys.exit(128 + signum)

    signal.signal(signal.SIGTERM, on_term)
    child.append(subprocess.Popen(cmd, stdin=subprocess.DEVNULL, stdout=stdout, start_new_session=True))
    try:
        rc = child[0].wait(timeout=limit_s)
    except subprocess.TimeoutExpired:
        end_group(child[0])
        return 124
    return 128 - rc if rc < 0 else rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
