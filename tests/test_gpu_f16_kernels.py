"""The kernel-level suites, run once more against the half-operand build (liboctmae_f16.so).

tests/test_gpu_f16_parity.py runs whole models on the half build; this module runs the kernel tests themselves -- every GEMM tile
variant, the split-K hand-off, the attention tail kernels, both backward forms, the delta epilogue, the weight-gradient pairs,
LayerNorm, the token plumbing, AdamW, the slice-pooling kernels, the operand-type edges of tests/test_gpu_lp_edges.py, the row-wise
attention checks of tests/test_gpu_attention_rows.py, the token / loss kernels of tests/test_gpu_tokens.py, the per-element GEMM bounds
and activation sweeps of tests/test_gpu_gemm_elements.py and the planted NaN / Inf of tests/test_gpu_nonfinite.py -- in a child
pytest process with OCTMAE_LIB pointing at the half build (the 16-bit type is chosen per process, before octcubem_amd is imported).

The child is started once the collection is known to contain a test of this module (tests/conftest.py::pytest_collection_finish ->
start_children()) through tests/children.py, which logs it to a file, runs it under a wall-clock limit and reaps it at exit; its
results go to a JUnit XML file.  The tests below read the XML: the child passed, every module ran at least as many tests as it holds today (a collection that
quietly shrinks fails), and every skip is on the allowlist.
"""
import os
import re
import sys
import xml.etree.ElementTree as ET

import pytest

from tests import children

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_F16 = os.path.join(ROOT, "octcubem_amd", "liboctmae_f16.so")
TIMEOUT_S = 1500

SUITES = ["tests/test_gpu_kernels.py", "tests/test_gpu_gemm_small.py",
          "tests/test_gpu_slicehead.py::test_slice_pool_kernels_vs_fp32_composition",
          "tests/test_gpu_slicehead.py::test_slice_pool_sidecar_matches_its_gradient",
          "tests/test_gpu_lp_edges.py", "tests/test_gpu_attention_rows.py", "tests/test_gpu_tokens.py",
          "tests/test_gpu_layernorm_rows.py", "tests/test_gpu_gemm_elements.py", "tests/test_gpu_nonfinite.py"]
# tests per module the child must run (passed + skipped), as collected with -m gpu when this module was written
MIN_TESTS = {"tests.test_gpu_kernels": 533, "tests.test_gpu_gemm_small": 20, "tests.test_gpu_slicehead": 37,
             "tests.test_gpu_lp_edges": 66, "tests.test_gpu_attention_rows": 21, "tests.test_gpu_tokens": 41,
             "tests.test_gpu_layernorm_rows": 116, "tests.test_gpu_gemm_elements": 423, "tests.test_gpu_nonfinite": 677}
# (test id, skip reason) pairs the half build may skip: none today
ALLOWED_SKIPS = set()

CHILD = "f16_kernels"


def _xml():
    return os.path.join(children.tmpdir(CHILD), "junit.xml")


def start_children():
    """The half-build child: a nested pytest session, one GPU process (nothing when the library is missing: _result() then fails with
    the build hint)."""
    if os.path.exists(LIB_F16):
        cmd = [sys.executable, "-m", "pytest", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider", f"--junitxml={_xml()}", *SUITES]
        children.spawn(CHILD, cmd, env=dict(os.environ, OCTMAE_LIB=LIB_F16), limit_s=TIMEOUT_S)


_RESULT = {}


def _log_tail(n=6000):
    return children.log_tail(CHILD, n)


def _result():
    if _RESULT:
        return _RESULT
    start_children()
    assert os.path.exists(LIB_F16), f"{LIB_F16} is missing: build it (python -c 'import __graft_entry__ as g; g.build()' or make -C octcubem_amd/csrc both)"
    rc = children.result(CHILD).rc
    if rc == 124:
        pytest.fail(f"the half-build kernel suite did not finish in {TIMEOUT_S} s:\n{_log_tail()}")
    cases = []
    if os.path.exists(_xml()):
        for tc in ET.parse(_xml()).getroot().iter("testcase"):
            status, msg = "passed", ""
            for kind in ("failure", "error", "skipped"):
                el = tc.find(kind)
                if el is not None:
                    status, msg = kind, el.get("message", "")
                    break
            cases.append((f"{tc.get('classname')}::{tc.get('name')}", status, msg))
    _RESULT.update(rc=rc, cases=cases)
    # the child's parity ledger (the u-scaled errors on half, printed by its session under -s) joins this session's, which
    # tests/conftest.py writes out at the end: one file holds both builds
    from tests import conftest
    m = re.search(r"^\[parity ledger\] (.*)$", _log_tail(None), re.M)
    for entry in (m.group(1).split("; ") if m else []):
        e = re.fullmatch(r"(\S+) (\S+) \(<= (\S+)\)", entry)
        if e:
            conftest._LEDGER.append((e.group(1), float(e.group(2)), float(e.group(3))))
    print(f"\n[half-build kernel suite] exit code {rc}: " +
          ", ".join(f"{mod} {c}" for mod, c in _counts(cases).items()))
    return _RESULT


def _module(case_id):
    return case_id.split("::")[0]


def _counts(cases):
    c = {}
    for cid, status, _ in cases:
        c.setdefault(_module(cid), {}).setdefault(status, 0)
        c[_module(cid)][status] += 1
    return c


def test_half_build_kernel_suite_passes():
    r = _result()
    bad = [cid for cid, status, _ in r["cases"] if status in ("failure", "error")]
    assert r["rc"] == 0 and not bad and r["cases"], (f"half build: exit code {r['rc']}, {len(bad)} failing:\n" + "\n".join(bad[:40]) +
                                                    f"\n--- child log ---\n{_log_tail()}")


def test_half_build_ran_every_kernel_module_in_full():
    r = _result()
    counts = _counts(r["cases"])
    short = {m: (sum(counts.get(m, {}).values()), n) for m, n in MIN_TESTS.items() if sum(counts.get(m, {}).values()) < n}
    assert not short, f"modules that ran fewer tests than they hold (ran, expected): {short}\n--- child log ---\n{_log_tail()}"


def test_half_build_skips_only_what_is_allowed():
    r = _result()
    skips = [(cid, msg) for cid, status, msg in r["cases"] if status == "skipped"]
    unexpected = [s for s in skips if s not in ALLOWED_SKIPS]
    assert not unexpected, "skips not on the allowlist:\n" + "\n".join(f"{c}: {m}" for c, m in unexpected) + f"\n--- child log ---\n{_log_tail(2000)}"
