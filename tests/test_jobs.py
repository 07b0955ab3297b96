"""Managed-jobs tests: controller recursion, recovery, cancellation,
checkpoint-backed resume contract (reference: SURVEY.md §2.7/§3.2)."""
import json
import os
import time
from pathlib import Path

import pytest

from tests.test_orchestrator import client, sky_env  # fixtures  # noqa: F401


def _wait_managed(job_id, statuses, timeout=90):
    from skypilot_amd.client import sdk
    deadline = time.time() + timeout
    last = None
    while time.time() < deadline:
        rows = sdk.get(sdk.jobs_queue())
        for r in rows:
            if r["job_id"] == job_id:
                last = r
                if r["status"] in statuses:
                    return r
        time.sleep(0.5)
    raise TimeoutError(f"managed job {job_id} last={last}")


def test_managed_job_success(client):
    from skypilot_amd.client import sdk
    task = {"name": "mj-ok", "run": "echo managed-ok"}
    res = sdk.get(sdk.jobs_launch(task, "mj-ok"))
    job = _wait_managed(res["job_id"], {"SUCCEEDED", "FAILED"})
    assert job["status"] == "SUCCEEDED"
    # Controller tore the job cluster down.
    deadline = time.time() + 30
    while time.time() < deadline:
        records = sdk.get(sdk.status())
        if not any(r["name"] == f"sky-jobs-{res['job_id']}"
                   for r in records):
            break
        time.sleep(0.5)
    else:
        pytest.fail("managed-job cluster not cleaned up")


def test_managed_job_restart_on_failure(client, tmp_path):
    """max_restarts_on_errors: first attempt exits 1, retry succeeds."""
    from skypilot_amd.client import sdk
    marker = tmp_path / "attempted"
    task = {
        "name": "mj-flaky",
        "resources": {"job_recovery": {"strategy": "FAILOVER",
                                       "max_restarts_on_errors": 2}},
        "run": f"if [ ! -f {marker} ]; then touch {marker}; exit 1; "
               "else echo recovered-ok; fi",
    }
    res = sdk.get(sdk.jobs_launch(task, "mj-flaky"))
    job = _wait_managed(res["job_id"], {"SUCCEEDED", "FAILED"}, timeout=120)
    assert job["status"] == "SUCCEEDED"
    assert job["recovery_count"] >= 1


def test_managed_job_failure_budget_exhausted(client):
    from skypilot_amd.client import sdk
    task = {"name": "mj-bad", "run": "exit 7"}  # no recovery budget
    res = sdk.get(sdk.jobs_launch(task, "mj-bad"))
    job = _wait_managed(res["job_id"], {"SUCCEEDED", "FAILED"}, timeout=120)
    assert job["status"] == "FAILED"


def test_managed_job_cancel(client):
    import subprocess
    import time as _t
    from skypilot_amd.client import sdk
    task = {"name": "mj-sleep", "run": "sleep 600"}
    res = sdk.get(sdk.jobs_launch(task, "mj-sleep"))
    _wait_managed(res["job_id"], {"RUNNING"})
    n = sdk.get(sdk.jobs_cancel([res["job_id"]]))
    assert n == 1
    job = _wait_managed(res["job_id"], {"CANCELLED"})
    assert job["status"] == "CANCELLED"
    # no leaked driver: cancel + teardown must reap the job driver
    # process (it runs in its own session and used to survive)
    import os
    home = os.environ["SKY_AMD_HOME"]
    deadline = _t.time() + 30
    while _t.time() < deadline:
        out = subprocess.run(
            ["ps", "-eo", "args"], capture_output=True, text=True).stdout
        leaked = [ln for ln in out.splitlines()
                  if "skypilot_amd.agent.driver" in ln and home in ln]
        if not leaked:
            break
        _t.sleep(1)
    assert not leaked, leaked


def test_managed_job_preemption_recovery(client, tmp_path):
    """Kill the job's cluster under the controller: it must detect the
    preemption, relaunch, and the task resumes from its mounted state
    (the checkpoint contract)."""
    from skypilot_amd.client import sdk
    ckpt = tmp_path / "ckpt"
    task = {
        "name": "mj-preempt",
        "file_mounts": {str(ckpt): {"name": "mj-preempt-ckpt",
                                    "mode": "MOUNT"}},
        # First incarnation sleeps (gets preempted); after recovery the
        # state file exists and it finishes immediately.
        "run": f"if [ -f {ckpt}/state ]; then echo resumed-from-ckpt; "
               f"else echo phase1 > {ckpt}/state; sleep 600; fi",
    }
    res = sdk.get(sdk.jobs_launch(task, "mj-preempt"))
    job_id = res["job_id"]
    _wait_managed(job_id, {"RUNNING"})
    time.sleep(2)  # let phase1 write its state
    # Preempt: tear the managed cluster down out from under the controller.
    cluster = f"sky-jobs-{job_id}"
    sdk.get(sdk.down(cluster))
    job = _wait_managed(job_id, {"SUCCEEDED", "FAILED"}, timeout=120)
    assert job["status"] == "SUCCEEDED"
    assert job["recovery_count"] >= 1
    # The mounted store kept phase1's state across the preemption.
    home = Path(os.environ["SKY_AMD_HOME"])
    assert (home / "storage" / "mj-preempt-ckpt" / "state").exists()


def test_managed_job_pipeline(client, tmp_path):
    """Chained tasks run sequentially on the controller (reference:
    pipelines via chained DAGs)."""
    from skypilot_amd.client import sdk
    out = tmp_path / "pipe.txt"
    task = {
        "name": "mj-pipe",
        "tasks": [
            {"name": "stage1", "run": f"echo one >> {out}"},
            {"name": "stage2", "run": f"echo two >> {out}"},
        ],
    }
    res = sdk.get(sdk.jobs_launch(task, "mj-pipe"))
    job = _wait_managed(res["job_id"], {"SUCCEEDED", "FAILED"}, timeout=120)
    assert job["status"] == "SUCCEEDED"
    assert out.read_text().split() == ["one", "two"]


def test_jobs_pool(client, tmp_path):
    """Pool workers: warm clusters; pooled jobs exec on free workers and
    queue when the pool is busy (reference: sky jobs pool, App. C)."""
    from skypilot_amd.client import sdk
    template = {"name": "pool-tmpl", "resources": {}}
    res = sdk.get(sdk.jobs_pool_apply("p1", template, 1), timeout=90)
    assert len(res["workers"]) == 1

    out = tmp_path / "pool-out.txt"
    j1 = sdk.get(sdk.jobs_launch(
        {"name": "pj1", "pool": "p1",
         "run": f"echo first >> {out}; sleep 3"}))
    j2 = sdk.get(sdk.jobs_launch(
        {"name": "pj2", "pool": "p1", "run": f"echo second >> {out}"}))
    r1 = _wait_managed(j1["job_id"], {"SUCCEEDED", "FAILED"}, timeout=120)
    r2 = _wait_managed(j2["job_id"], {"SUCCEEDED", "FAILED"}, timeout=120)
    assert r1["status"] == "SUCCEEDED" and r2["status"] == "SUCCEEDED"
    # One worker => serialized: first finished before second started.
    assert out.read_text().split() == ["first", "second"]
    st = sdk.get(sdk.jobs_pool_status("p1"))
    assert st[0]["workers"][0]["status"] == "READY"
    # Worker cluster survives the jobs (warm pool).
    records = sdk.get(sdk.status())
    assert any(r["name"] == "sky-pool-p1-0" for r in records)
    sdk.get(sdk.jobs_pool_down("p1"))
    records = sdk.get(sdk.status())
    assert not any(r["name"].startswith("sky-pool-p1") for r in records)


def test_managed_spot_job_recovers_after_preemption(client, tmp_path):
    """Spot end-to-end: a use_spot managed job loses its GPUs to an
    on-demand launch (true capacity preemption, not a manual kill),
    enters RECOVERING, and finishes once capacity frees up."""
    from skypilot_amd.client import sdk
    ckpt = tmp_path / "spot-ckpt"
    task = {
        "name": "mj-spot",
        "resources": {"accelerators": "MI355X:6", "use_spot": True},
        "file_mounts": {str(ckpt): {"name": "mj-spot-ckpt",
                                    "mode": "MOUNT"}},
        "run": f"if [ -f {ckpt}/state ]; then echo resumed; "
               f"else echo phase1 > {ckpt}/state; sleep 600; fi",
    }
    res = sdk.get(sdk.jobs_launch(task, "mj-spot"))
    job_id = res["job_id"]
    _wait_managed(job_id, {"RUNNING"})
    time.sleep(2)
    # On-demand launch takes the GPUs -> the spot cluster is reclaimed.
    sdk.get(sdk.launch({"run": "true",
                        "resources": {"accelerators": "MI355X:4"}},
                       "od-grab"), timeout=60)
    # Spot job must notice and recover; capacity frees when od-grab downs.
    sdk.get(sdk.down("od-grab"))
    job = _wait_managed(job_id, {"SUCCEEDED", "FAILED"}, timeout=180)
    assert job["status"] == "SUCCEEDED", job
    assert job["recovery_count"] >= 1


def test_recover_on_exit_codes(client, tmp_path):
    """Exit codes listed in job_recovery.recover_on_exit_codes recover
    without consuming the restart budget (reference: schema field)."""
    from skypilot_amd.client import sdk
    # exit 42 twice (recover_on_exit_codes, no budget needed), then 0.
    # The counter lives in this test's own directory: a fixed name in a
    # shared temp dir may already exist and belong to another user.
    marker = str(tmp_path / "roec-count")
    task = {
        "name": "mj-roec",
        "resources": {"job_recovery": {"strategy": "EAGER",
                                       "recover_on_exit_codes": [42],
                                       "max_restarts_on_errors": 0}},
        "run": f"n=$(cat {marker} 2>/dev/null || echo 0); "
               f"echo $((n+1)) > {marker}; "
               f"if [ $n -lt 2 ]; then exit 42; fi",
    }
    res = sdk.get(sdk.jobs_launch(task, "mj-roec"))
    job = _wait_managed(res["job_id"], {"SUCCEEDED", "FAILED"},
                        timeout=180)
    assert job["status"] == "SUCCEEDED", job
    assert job["recovery_count"] >= 2


def test_job_group_concurrent_colocated(client, tmp_path):
    """JobGroup (reference: jobs/job_group_networking.py): members run
    CONCURRENTLY on one shared cluster with group addressing env."""
    from skypilot_amd.client import sdk
    d = tmp_path / "grp"
    d.mkdir()
    # Each member writes its group env, then waits for the OTHER's file
    # — only concurrent execution on one cluster lets both finish.
    def run(me, other):
        return (f"env | grep SKYPILOT_JOBGROUP > {d}/{me}.env; "
                f"for i in $(seq 1 100); do "
                f"[ -f {d}/{other}.env ] && exit 0; sleep 0.2; done; "
                f"exit 1")
    res = sdk.get(sdk.jobs_group_launch("g1", [
        {"name": "ps", "run": run("ps", "worker"),
         "resources": {"accelerators": "MI355X:2"}},
        {"name": "worker", "run": run("worker", "ps"),
         "resources": {"accelerators": "MI355X:2"}},
    ]), timeout=120)
    assert res["cluster"] == "sky-group-g1"
    assert len(res["members"]) == 2
    deadline = time.time() + 90
    while time.time() < deadline:
        st = sdk.get(sdk.jobs_group_status("g1"))
        if all(m["status"] in ("SUCCEEDED", "FAILED", "CANCELLED")
               for m in st["members"]):
            break
        time.sleep(1)
    assert all(m["status"] == "SUCCEEDED" for m in st["members"]), st
    ps_env = (d / "ps.env").read_text()
    assert "SKYPILOT_JOBGROUP_NAME=g1" in ps_env
    assert "SKYPILOT_JOBGROUP_TASK=ps" in ps_env
    assert "SKYPILOT_JOBGROUP_HOST=127.0.0.1" in ps_env
    assert "SKYPILOT_JOBGROUP_TASKS=ps,worker" in ps_env
    sdk.get(sdk.jobs_group_down("g1"))


def test_controller_concurrency_capped(sky_env, client, monkeypatch):
    """With SKY_AMD_MAX_CONTROLLERS=2, launching 6 managed jobs keeps at
    most 2 controller processes alive at any time and all 6 complete
    (reference: sky/jobs/scheduler.py:232 maybe_start_controllers)."""
    import time
    from skypilot_amd.client import sdk
    from skypilot_amd.jobs import scheduler, state
    monkeypatch.setenv("SKY_AMD_MAX_CONTROLLERS", "2")
    ids = []
    for i in range(6):
        r = sdk.get(sdk.jobs_launch({"run": "sleep 0.4",
                                     "resources": {"cpus": 1}},
                                    name=f"cap-{i}"), timeout=60)
        ids.append(r["job_id"])
    max_live = 0
    deadline = time.time() + 180
    while time.time() < deadline:
        jobs = {j["job_id"]: j for j in state.list_jobs()}
        live = sum(1 for j in jobs.values()
                   if j["status"] not in state.TERMINAL
                   and scheduler._pid_alive(j.get("controller_pid")))
        max_live = max(max_live, live)
        done = sum(1 for i in ids if jobs[i]["status"] in state.TERMINAL)
        if done == 6:
            break
        scheduler.maybe_start_controllers()  # belt-and-braces drain
        time.sleep(0.3)
    jobs = {j["job_id"]: j for j in state.list_jobs()}
    assert all(jobs[i]["status"] == "SUCCEEDED" for i in ids), jobs
    assert max_live <= 2, max_live


def test_mount_cached_remote_checkpoint_recovery(sky_env, client,
                                                 monkeypatch, tmp_path):
    """MOUNT_CACHED with a remote bucket is a real rclone FUSE mount
    with VFS write-back (reference: mounting_utils.py:698, VERDICT r01
    #8).  A faked rclone simulates mount (bind via symlink) + sync:
    write a checkpoint through the mount, tear the cluster down,
    re-mount on a fresh cluster, and the checkpoint is there."""
    import stat
    # fake rclone: "mount remote:path target --daemon ..." symlinks the
    # backing dir; other verbs no-op.  (Real boxes use real rclone.)
    backing = tmp_path / "bucket"
    backing.mkdir()
    fake_bin = tmp_path / "bin"
    fake_bin.mkdir()
    rc = fake_bin / "rclone"
    rc.write_text(f"""#!/bin/bash
if [ "$1" = mount ]; then
  tgt="$3"
  rmdir "$tgt" 2>/dev/null || true
  ln -sfn {backing} "$tgt"
  exit 0
fi
exit 0
""")
    rc.chmod(rc.stat().st_mode | stat.S_IEXEC)
    monkeypatch.setenv("PATH", f"{fake_bin}:{os.environ['PATH']}")
    # fusermount absent -> unmount is best-effort; symlink removal via
    # rmtree is fine for the fake.
    from skypilot_amd.client import sdk
    mnt = str(tmp_path / "ckpt-mnt")
    mount = {mnt: {"name": "ckpt-bkt", "mode": "MOUNT_CACHED",
                   "source": "s3://bkt/ck"}}
    sdk.get(sdk.launch({"run": f"echo step-500 > {mnt}/model.ck",
                        "file_mounts": mount,
                        "resources": {"cpus": 1}}, "mc-1"), timeout=60)
    from tests.test_orchestrator import _wait_job_done
    assert _wait_job_done("mc-1", 1)["status"] == "SUCCEEDED"
    assert (backing / "model.ck").read_text().strip() == "step-500"
    sdk.get(sdk.down("mc-1"))
    # recovery: a fresh cluster re-mounts the same bucket and resumes
    sdk.get(sdk.launch({"run": f"cat {mnt}/model.ck",
                        "file_mounts": mount,
                        "resources": {"cpus": 1}}, "mc-2"), timeout=60)
    j = _wait_job_done("mc-2", 1)
    assert j["status"] == "SUCCEEDED"
    sdk.get(sdk.down("mc-2"))


def test_controller_log_gc(sky_env, client):
    """Old terminal-job controller logs are garbage-collected
    (reference: sky/jobs/log_gc.py retention)."""
    import os
    from skypilot_amd.client import sdk
    from skypilot_amd.jobs import state
    from skypilot_amd.server.daemons import _gc_controller_logs
    r = sdk.get(sdk.jobs_launch({"run": "true",
                                 "resources": {"cpus": 1}},
                                name="gc-job"), timeout=60)
    jid = r["job_id"]
    deadline = time.time() + 120
    while time.time() < deadline:
        j = state.get(jid)
        if j and j["status"] in state.TERMINAL:
            break
        time.sleep(0.3)
    log = state.global_state.root_dir() / f"jobs-controller-{jid}.log"
    assert log.exists()
    # fresh logs stay
    assert _gc_controller_logs(max_age_days=7) == 0
    assert log.exists()
    # age it and collect
    old = time.time() - 8 * 86400
    os.utime(log, (old, old))
    assert _gc_controller_logs(max_age_days=7) >= 1
    assert not log.exists()
