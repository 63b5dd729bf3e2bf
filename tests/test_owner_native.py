"""Host sanitizers on the owning types of der-vet_amd/csrc/dvh_host.h (DevBuf, DevEvent, PinnedBuf):
tests/native/owner_sanitize.cpp, a stand-alone program with counting stand-ins of the six HIP calls they make, built
with -fsanitize=address,undefined (no recovery) as tests/test_sizing_sanitize.py builds its driver.  CPU only: creates
and destroys balance, a moved-from object releases nothing, the chunk-event pool's growth destroys each event once, a
failed create leaves the object empty and reusable, DevBuf::ensure keeps its grow-only and slack behaviour -- with no
sanitizer report."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHECKS = ["lazy_nothing_made", "ensure_creates_once", "scope_end_balances", "move_construct_takes",
          "move_assign_releases_own_only", "self_move_keeps", "moved_to_released_once", "moved_from_is_reusable",
          "moves_balance", "vector_growth_moves", "vector_destroys_each_once", "failed_create_leaves_empty",
          "failed_create_is_retried", "failures_balance", "devbuf_zero_request", "devbuf_floor_256",
          "devbuf_keeps_when_it_fits", "devbuf_grows_exactly", "devbuf_never_shrinks", "devbuf_slack",
          "devbuf_slack_on_growth_only", "devbuf_release_empties", "devbuf_balances"]


@pytest.fixture(scope="module")
def sanitized_run(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("asan") / "owner_sanitize")
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-o", exe,
           os.path.join(ROOT, "tests", "native", "owner_sanitize.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)


def test_sanitized_run_is_clean(sanitized_run):
    p = sanitized_run
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-6000:]
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-6000:]
    assert p.stdout.rstrip().endswith("done") and "failures=0" in p.stdout


@pytest.mark.parametrize("check", CHECKS)
def test_owner_property_holds(sanitized_run, check):
    assert re.search(rf"^{check} ok$", sanitized_run.stdout, re.M), sanitized_run.stdout[-2500:]
