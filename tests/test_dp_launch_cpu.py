"""tests/dp_launch.py without a GPU: the children are tiny `python -c` programs (no torch) that write their pid into the output directory
first, so the parent can see afterwards that none of them is left."""
import os
import time

import pytest

from dp_launch import ROOT, run_ranks, world2_env

PID = "import os, sys, time\nr = os.environ['RANK']\nopen(os.path.join(sys.argv[1], 'pid' + r), 'w').write(str(os.getpid()))\n"


def gone(out, r):
    with open(os.path.join(out, f"pid{r}")) as fh:
        pid = int(fh.read())
    try:
        os.kill(pid, 0)
    except ProcessLookupError:
        return True
    return False


def test_two_ranks_exit_0_and_see_their_own_environment(tmp_path):
    prog = PID + "print(r, os.environ['LOCAL_RANK'], os.environ['WORLD_SIZE'], os.environ['MASTER_PORT'], sys.argv[2])\n"
    logs = run_ranks(["-c", prog], str(tmp_path), timeout=30, extra_args=("extra",))
    seen = [lg.split() for lg in logs]
    assert [s[:3] for s in seen] == [["0", "0", "2"], ["1", "1", "2"]]
    assert seen[0][3] == seen[1][3] and int(seen[0][3]) > 0 and seen[0][4] == seen[1][4] == "extra"
    for r in range(2):
        with open(tmp_path / f"rank{r}.log") as fh:
            assert fh.read() == logs[r]
        assert gone(str(tmp_path), r)


def test_a_failed_rank_ends_its_peer_after_the_grace_period(tmp_path):
    prog = PID + "if r == '1':\n    print('rank one says no')\n    sys.exit(3)\ntime.sleep(60)\n"
    t0 = time.monotonic()
    with pytest.raises(AssertionError) as err:
        run_ranks(["-c", prog], str(tmp_path), peer_grace=1)
    assert time.monotonic() - t0 < 5
    text = str(err.value)
    assert "rank 1: exit code 3" in text and "rank one says no" in text and "killed after rank 1 failed" in text
    assert gone(str(tmp_path), 0) and gone(str(tmp_path), 1)


def test_the_time_limit_ends_both_ranks(tmp_path):
    t0 = time.monotonic()
    with pytest.raises(AssertionError) as err:
        run_ranks(["-c", PID + "time.sleep(60)\n"], str(tmp_path), timeout=2)
    assert time.monotonic() - t0 < 6
    assert str(err.value).count("time limit") == 2
    assert gone(str(tmp_path), 0) and gone(str(tmp_path), 1)


def test_two_mebibytes_of_output_do_not_block_a_rank(tmp_path):
    prog = PID + "for i in range(32768):\n    print('%063d' % i)\nprint('last line of rank', r)\n"
    logs = run_ranks(["-c", prog], str(tmp_path), timeout=30)
    for r, lg in enumerate(logs):
        assert len(lg) > 2 * 1024 * 1024 and lg.endswith(f"last line of rank {r}\n")


def test_world2_env_is_the_set_the_fixtures_used(monkeypatch):
    monkeypatch.setattr(os, "environ", {"KEPT": "1"})
    env = world2_env()
    port = env.pop("MASTER_PORT")
    assert 0 < int(port) < 65536
    assert env == {"KEPT": "1", "MASTER_ADDR": "127.0.0.1", "WORLD_SIZE": "2", "NEF_DIST_BACKEND": "gloo", "NEF_SHARE_GPU": "1",
                   "NEF_TEST_HOOKS": "1", "PYTHONPATH": ROOT, "HSA_ENABLE_IPC_MODE_LEGACY": "0"}
    bare = world2_env(share_gpu=False)
    assert set(bare) == (set(env) | {"MASTER_PORT"}) - {"NEF_DIST_BACKEND", "NEF_SHARE_GPU"}
    assert all(bare[k] == env[k] for k in bare if k != "MASTER_PORT")
