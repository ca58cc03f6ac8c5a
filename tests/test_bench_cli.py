"""CPU: bench.py's command line -- a plain run is the headline leg alone; the extras sit behind --full."""
import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr("sys.argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_lean_by_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert not a.full and a.dump_outputs is None and (a.steps, a.warmup, a.gpus) == (7, 2, 1)


def test_full_and_dump_outputs_options(monkeypatch):
    a = _parse(monkeypatch, "--full", "--dump-outputs", "out", "--no-policy")
    assert a.full and a.dump_outputs == "out" and a.no_policy and not a.no_train
