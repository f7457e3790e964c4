"""ray_amd.init options honoured or rejected (reference: ray.init): unknown keywords raise,
_system_config keys map onto the raylet's RAY_<key> settings (unknown keys raise),
log_to_driver=False keeps worker output out of the driver terminal (it still lands in the
per-worker log files), storage sets the default results storage, logging_level is applied."""
import glob
import logging
import os
import subprocess
import sys
import textwrap

import pytest

import ray_amd as ray


def test_unknown_keyword_and_system_config_validation():
    with pytest.raises(TypeError, match="unexpected keyword"):
        ray.init(num_cpus=1, no_such_option=1)
    with pytest.raises(ValueError, match="unsupported _system_config key"):
        ray.init(num_cpus=1, _system_config={"made_up": 1})
    assert not ray.is_initialized()


def _run(code):
    return subprocess.run([sys.executable, "-c", textwrap.dedent(code)], capture_output=True,
                          text=True, timeout=120, cwd=os.getcwd(),
                          env=dict(os.environ, PYTHONPATH=os.getcwd()))


def test_log_to_driver_false_and_system_config(tmp_path):
    code = f"""
    import glob, os, time, logging
    import ray_amd as ray
    ctx = ray.init(num_cpus=1, log_to_driver=False, logging_level=logging.DEBUG,
                   storage={str(tmp_path)!r},
                   _system_config={{"memory_usage_threshold": 0.99}})

    @ray.remote
    def hello():
        print("WORKER-SAYS-HI", flush=True)
        return os.environ.get("RAY_memory_usage_threshold")

    print("threshold", ray.get(hello.remote()))
    print("level", logging.getLogger("ray_amd").level)
    print("storage", os.environ.get("RAY_AMD_STORAGE"))
    time.sleep(0.5)
    logs = glob.glob(os.path.join(ctx["session_dir"], "logs", "worker-*.out"))
    print("in_files", any("WORKER-SAYS-HI" in open(p).read() for p in logs))
    ray.shutdown()
    """
    r = _run(code)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "WORKER-SAYS-HI" not in r.stdout.replace("in_files", "")
    assert "threshold 0.99" in r.stdout  # the raylet (and its workers) got RAY_<key>
    assert f"level {logging.DEBUG}" in r.stdout
    assert f"storage {tmp_path}" in r.stdout
    assert "in_files True" in r.stdout


def test_session_root_fits_worker_sockets_and_is_ours(tmp_path, monkeypatch):
    """Session directories go to <tempdir>/ray_amd_sessions unless the raylet and worker
    sockets below it would not fit an AF_UNIX path (a long TMPDIR: /tmp instead) or another
    user owns that directory (not writable for us: ray_amd_<uid> beside it instead).
    RAY_AMD_TMPDIR is taken as given."""
    import tempfile

    from ray_amd._private import worker as W

    sock = "/session_2000-01-01_00-00-00_1234567_abcdef/sockets/" + "0" * 24 + ".sock"
    monkeypatch.delenv("RAY_AMD_TMPDIR", raising=False)
    uid = os.getuid()
    long_tmp = tmp_path / ("d" * 60)
    long_tmp.mkdir()
    monkeypatch.setattr(tempfile, "tempdir", str(long_tmp))
    root = W._session_root()
    assert root in ("/tmp/ray_amd_sessions", f"/tmp/ray_amd_{uid}")
    assert len(root + sock) <= 107
    # a temp dir that leaves room is used as it is; the shared name while nobody else owns it
    short = str(tmp_path / "s")
    os.mkdir(short)
    monkeypatch.setattr(W, "_ROOT_MAX", len(short + "/ray_amd_sessions"))
    monkeypatch.setattr(tempfile, "tempdir", short)
    assert W._session_root() == short + "/ray_amd_sessions"
    os.mkdir(short + "/ray_amd_sessions")
    assert W._session_root() == short + "/ray_amd_sessions"  # ours
    monkeypatch.setattr(os, "getuid", lambda: uid + 1)  # now it is another user's directory
    assert W._session_root() == short + f"/ray_amd_{uid + 1}"
    monkeypatch.setenv("RAY_AMD_TMPDIR", str(long_tmp))
    assert W._session_root() == str(long_tmp)
