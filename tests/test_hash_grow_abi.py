"""sgk_tabq_hash_grow (include/sgk.h) -- the hashed Q-tables rehashed into larger ones on the device -- as far as a box without a GPU
can tell: the symbol is declared, exported and bound with the header's signature, a call that cannot be right is refused with a
message before anything touches a device, and the trainer's --hash-grow parses, is absent unless given and stops a run on a level
whose tables are not hashed."""
import ctypes
import os
import re

import pytest

from safe_grid_agents_amd import _lib, agents, trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbol_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "sgk.h")).read()
    m = re.search(r"SGK_API\s+int\s+sgk_tabq_hash_grow\s*\(([^)]*)\)\s*;", text)
    assert m, "include/sgk.h does not declare sgk_tabq_hash_grow"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["sgk_tabq *q", "int32_t new_capacity"]
    assert "sgk_tabq_hash_grow" in _lib.EXPORTED_SYMBOLS
    res, args = _lib._SIGNATURES["sgk_tabq_hash_grow"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_int32]
    lib = _lib.load()
    assert lib.sgk_tabq_hash_grow.argtypes == args
    assert lib.sgk_abi_version() == 4  # an added symbol: the ABI version stays
    assert re.search(r"#define\s+SGK_ABI_VERSION\s+4\b", text)


def test_a_null_handle_is_refused_with_a_message():
    lib = _lib.load()
    for capacity in (128, 64, 0, -1, 96, 1 << 25):
        assert lib.sgk_tabq_hash_grow(None, capacity) == _lib.ERR_INVALID, capacity
        msg = lib.sgk_last_error()
        assert msg and b"NULL" in msg, (capacity, msg)


def test_the_batched_agent_offers_growth():
    A = agents.BatchedTabularQAgent
    assert callable(getattr(A, "grow_hash", None)) and callable(getattr(A, "reserve_hash", None))


def _parse(*argv):
    return trainer.prepare_parser().parse_args(list(argv))


def test_hash_grow_parses_and_is_absent_unless_given():
    args = _parse("-N", "8", "tomato", "tabular-q", "-l", "0.4", "--hash-grow")
    assert args.hash_grow is True and trainer.check_hash_grow(args) is True
    assert _parse("-N", "8", "tomato", "tabular-q", "-l", "0.4", "-HG").hash_grow is True
    args = _parse("-N", "8", "tomato", "tabular-q", "-l", "0.4")
    assert "hash_grow" not in vars(args) and trainer.check_hash_grow(args) is False
    with pytest.raises(SystemExit):  # the flag belongs to tabular-q: another agent's grammar does not know it
        _parse("-N", "8", "tomato", "random", "--hash-grow")


@pytest.mark.parametrize("env_alias", ["island", "sokoban", "boat"])
def test_another_level_than_tomato_stops_with_the_message(env_alias):
    args = _parse("-N", "8", env_alias, "tabular-q", "-l", "0.4", "--hash-grow")
    with pytest.raises(SystemExit) as e:
        trainer.check_hash_grow(args)
    assert "--hash-grow runs on tomato only" in str(e.value) and env_alias in str(e.value)
    with pytest.raises(SystemExit) as e:  # and train_batched stops there, before it makes an env
        trainer.train_batched(args)
    assert "--hash-grow runs on tomato only" in str(e.value)
