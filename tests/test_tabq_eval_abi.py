"""sgk_tabq_eval (include/sgk.h) -- default_eval for the batched tabular-Q agents in one launch -- as far as a box without a GPU can
tell: the symbol is declared, exported and bound with the header's signature, arguments that cannot be right are refused with a
message before anything touches a device, and the Python layer offers the fused path (BatchedTabularQAgent.evaluate / fused_eval,
taken by loops.batched_default_eval)."""
import ctypes
import os
import re

from safe_grid_agents_amd import _lib, agents, loops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbol_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "sgk.h")).read()
    m = re.search(r"SGK_API\s+int\s+sgk_tabq_eval\s*\(([^)]*)\)\s*;", text)
    assert m, "include/sgk.h does not declare sgk_tabq_eval"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["sgk_tabq *q", "int64_t n_reset_steps", "int64_t n_tail_steps", "int kernel"]
    assert "sgk_tabq_eval" in _lib.EXPORTED_SYMBOLS
    res, args = _lib._SIGNATURES["sgk_tabq_eval"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]
    lib = _lib.load()
    assert lib.sgk_tabq_eval.argtypes == args
    assert lib.sgk_abi_version() == 4  # an added symbol: the ABI version stays


def test_calls_that_cannot_be_right_are_refused_with_a_message():
    """Without a GPU there is no handle to give: a NULL handle is refused whatever else is passed -- negative counts and an unknown
    kernel included --, with a message, before anything touches a device. (tests/test_gpu_tabq_eval.py makes the same calls on a
    valid handle and reads which argument the message names.)"""
    lib = _lib.load()
    for call in [(None, 5, 7, _lib.TABQ_KERNEL_AUTO), (None, 0, 0, _lib.TABQ_KERNEL_AUTO), (None, -1, 7, _lib.TABQ_KERNEL_AUTO),
                 (None, 5, -1, _lib.TABQ_KERNEL_HBM), (None, -2**62, -2**62, _lib.TABQ_KERNEL_LDS), (None, 5, 7, 3), (None, 5, 7, -1)]:
        assert lib.sgk_tabq_eval(*call) == _lib.ERR_INVALID, call
        msg = lib.sgk_last_error()
        assert msg and b"NULL" in msg, (call, msg)


def test_the_batched_agent_offers_the_fused_evaluation():
    A = agents.BatchedTabularQAgent
    assert callable(getattr(A, "evaluate", None)) and callable(getattr(A, "evaluate_enqueue", None))
    assert A.fused_eval is True


def test_batched_default_eval_takes_the_fused_path_only_when_asked():
    """fused_eval = True: one agent.evaluate() call and nothing else; False: the loop of per-step calls, as before."""
    calls = []

    class Info:
        max_iterations = 3

    class Env:
        info, reward_scale = Info(), 1.0

        def metrics_reset(self): calls.append("metrics_reset")
        def reset(self): calls.append("reset")
        def reset_done(self): calls.append("reset_done")
        def step(self, actions, auto_reset=False, write_boards=True): calls.append("step")
        def metrics(self): return [0] * _lib.METRICS_LEN

    class Agent:
        fused_eval = True

        def act(self): calls.append("act"); return None
        def evaluate(self, eval_timesteps): calls.append(("evaluate", eval_timesteps)); return "fused"

    agent = Agent()
    assert loops.batched_default_eval(agent, Env(), 4) == "fused" and calls == [("evaluate", 4)]
    del calls[:]
    agent.fused_eval = False
    bm = loops.batched_default_eval(agent, Env(), 4)
    assert bm.episodes == 0
    assert calls == ["metrics_reset", "reset"] + ["act", "step", "reset_done"] * 3 + ["act", "step"] * 3
