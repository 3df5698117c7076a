"""bench.py's options, without a GPU: --full and --dump-outputs exist, and the
legs beside the headline are off unless --full is given."""
import sys

import bench


def parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None


def test_full_and_dump_outputs(monkeypatch, tmp_path):
    a = parse(monkeypatch, "--full", "--dump-outputs", str(tmp_path))
    assert a.full is True and a.dump_outputs == str(tmp_path)


def test_dump_fits_its_budget():
    # per-key sizes of 2^20 keys as float32, and room left for the state ranges
    assert 4 * 4 * bench.DUMP_KEY_SIZE_KEYS < bench.DUMP_BUDGET <= 64_000_000
