"""Ensemble acting for the conv bodies (include/sgk.h: sgk_convq_act_members_all, sgk_members_act_out; BatchedPPOCNNPopulation's
ensemble_act / evaluate_ensemble) as far as a box without a GPU can tell: the symbol is declared, exported and bound with the header's
signature and the ABI version stays; every bad argument is refused before the handle is looked at, with a message, and nothing is
written; the Python wrapper turns a tensor of the wrong device, dtype or shape into a ValueError before it reaches the library; every
field of the output descriptor names a guard-band test of tests/test_gpu_convq_ensemble.py; the population has the two methods and the
command line still refuses ppo-cnn."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import safe_grid_agents_amd as S
from safe_grid_agents_amd import _lib, ensemble
from safe_grid_agents_amd.envs import BatchedGridworldEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, I32 = ctypes.c_void_p, ctypes.c_int32
WEIGHT_NAMES = ("w1", "b1", "w2", "b2", "wb", "bb", "wh", "bh", "wl", "bl")

# Every pointer of sgk_members_act_out the library writes through -> the guard-band tests of tests/test_gpu_convq_ensemble.py that carve
# it from a guard_arena.Arena. (The descriptor is passed by const pointer, so tests/test_guard_arena_cpu.py's parser does not see its
# fields; this table is that file's COVERED for them until the struct is listed there.)
ACT_OUT_COVERED = {
    "sgk_members_act_out.member_actions_dev": ("test_gpu_convq_ensemble.test_the_outputs_stay_inside_their_guard_bands",),
    "sgk_members_act_out.member_scores_dev": ("test_gpu_convq_ensemble.test_the_outputs_stay_inside_their_guard_bands",),
}


def _header():
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "sgk.h")).read(), flags=re.S)


def _declared(name):
    m = re.search(r"SGK_API\s+int\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, "include/sgk.h does not declare int %s" % name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _struct_fields(name):
    """[(declaration, field name)] of a typedef'd struct of the header."""
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S)
    assert m, "include/sgk.h does not define %s" % name
    out = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if decl:
            out.append((decl, re.match(r".*?(\w+)$", decl).group(1)))
    return out


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_bound():
    assert _declared("sgk_convq_act_members_all") == ["sgk_env *h", "const sgk_convq_weights *w", "int32_t n_members",
                                                      "const sgk_members_act_out *out"]
    assert _struct_fields("sgk_members_act_out") == [("uint8_t *member_actions_dev", "member_actions_dev"),
                                                     ("float *member_scores_dev", "member_scores_dev")]
    want = (ctypes.c_int, [V, ctypes.POINTER(_lib.SgkConvQWeights), I32, ctypes.POINTER(_lib.SgkMembersActOut)])
    assert [k for k, _ in _lib.SgkMembersActOut._fields_] == ["member_actions_dev", "member_scores_dev"]
    assert ctypes.sizeof(_lib.SgkMembersActOut) == 2 * ctypes.sizeof(ctypes.c_void_p)
    lib = _lib.load()  # (resolves every bound symbol in libsgk.so: a missing export is an AttributeError here)
    assert "sgk_convq_act_members_all" in _lib.EXPORTED_SYMBOLS
    assert _lib._SIGNATURES["sgk_convq_act_members_all"] == want
    assert lib.sgk_convq_act_members_all.argtypes == want[1] and lib.sgk_convq_act_members_all.restype is want[0]
    assert lib.sgk_abi_version() == 4  # an added symbol: the ABI version stays
    raw = " ".join(open(os.path.join(ROOT, "include", "sgk.h")).read().split())
    assert "sgk_members_act_out is listed there" in raw and "test_guard_arena_cpu.py" in raw  # the header says why a descriptor


def _weights(blob, channels=5, layers=2, null=None):
    ptrs = [None if k == null else blob.ctypes.data for k in WEIGHT_NAMES]
    return _lib.SgkConvQWeights(*ptrs, channels, layers)


def test_every_bad_argument_is_refused_before_the_handle_and_nothing_is_written():
    """The handle is NULL in every call: a refusal that names the bad argument was made before the handle was looked at, so the same
    check guards a real handle. Valid arguments with a NULL handle are refused for the handle. The buffers are host memory that a
    launch would never be given; they keep their bytes."""
    lib = _lib.load()
    M, n = 3, 8
    actions, scores = np.full((M, n), 9, dtype=np.uint8), np.full((M, n, 4), 2.5, dtype=np.float32)
    blob = np.zeros(64, dtype=np.float32)
    assert scores.ctypes.data % 16 == 0
    w = _weights(blob)
    good = _lib.SgkMembersActOut(actions.ctypes.data, scores.ctypes.data)
    no_scores = _lib.SgkMembersActOut(actions.ctypes.data, None)
    cases = [
        ((None, M, ctypes.byref(good)), b"NULL argument"),
        ((ctypes.byref(w), M, None), b"out is NULL"),
        ((ctypes.byref(w), M, ctypes.byref(_lib.SgkMembersActOut(None, scores.ctypes.data))), b"member_actions_dev is NULL"),
        ((ctypes.byref(w), 0, ctypes.byref(good)), b"n_members"), ((ctypes.byref(w), -1, ctypes.byref(good)), b"n_members"),
        ((ctypes.byref(w), 4097, ctypes.byref(good)), b"n_members"),
        ((ctypes.byref(w), M, ctypes.byref(_lib.SgkMembersActOut(actions.ctypes.data, scores.ctypes.data + 4))), b"16-byte aligned"),
        ((ctypes.byref(w), M, ctypes.byref(_lib.SgkMembersActOut(actions.ctypes.data, scores.ctypes.data + 8))), b"16-byte aligned"),
        ((ctypes.byref(_weights(blob, channels=6)), M, ctypes.byref(good)), b"n_channels"),
        ((ctypes.byref(_weights(blob, channels=0)), M, ctypes.byref(good)), b"n_channels"),
        ((ctypes.byref(_weights(blob, layers=3)), M, ctypes.byref(good)), b"n_layers"),
    ]
    cases += [((ctypes.byref(_weights(blob, null=k)), M, ctypes.byref(good)), b"NULL argument") for k in WEIGHT_NAMES]
    for args, message in cases:
        assert lib.sgk_convq_act_members_all(None, *args) == _lib.ERR_INVALID, message
        assert message in lib.sgk_last_error(), (message, lib.sgk_last_error())
    for channels in (4, 5, 8):  # valid arguments, the optional output absent or present, 1 and 4096 members: only the handle is missing
        for out in (good, no_scores):
            for members in (1, M, 4096):
                assert lib.sgk_convq_act_members_all(None, ctypes.byref(_weights(blob, channels)), members, ctypes.byref(out)) == _lib.ERR_INVALID
                assert b"handle is NULL" in lib.sgk_last_error()
    assert (actions == 9).all() and (scores == 2.5).all()


# ---- the Python wrapper -----------------------------------------------------------------------------------------------------------------
class _OnDevice0(torch.Tensor):
    """A host tensor that reports cuda:0 as its device: the wrapper's checks read device, dtype, shape and contiguity and raise before
    any pointer is taken, so its dtype and shape refusals can be met without a GPU."""
    device = property(lambda self: torch.device("cuda", 0))


def _dev(t):
    return t.as_subclass(_OnDevice0)


def _stub_env(n_envs=10, cells=25):
    """The attributes convq_act_members_all reads before it calls the library (which a ValueError never reaches)."""
    env = object.__new__(BatchedGridworldEnv)
    env.device, env.n_envs, env.n_cells = 0, n_envs, cells
    return env


def _stacked(M, C, cells, wrap=_dev):
    shapes = {"w1": (M, C, 1, 3, 3), "b1": (M, C), "w2": (M, C, C, 3, 3), "b2": (M, C), "wb": (M, C, 1, 1, 1), "bb": (M, C),
              "wh": (M, C, C, 3, 3), "bh": (M, C), "wl": (M, 4, C * cells), "bl": (M, 4)}
    return {k: wrap(torch.zeros(s, dtype=torch.float32)) for k, s in shapes.items()}


def test_the_wrapper_refuses_a_wrong_tensor_with_a_value_error():
    M, C, n, cells = 3, 5, 10, 25
    env = _stub_env(n, cells)
    w = _stacked(M, C, cells)
    assert w["w1"].device == torch.device("cuda", 0) and isinstance(w["w1"], torch.Tensor)
    out, scores = _dev(torch.zeros((M, n), dtype=torch.uint8)), _dev(torch.zeros((M, n, 4), dtype=torch.float32))

    def but(k, t):
        d = dict(w)
        d[k] = t
        return d

    cases = [
        (dict(weights=w, n_members=0), "n_members"), (dict(weights=w, n_members=4097), "n_members"),
        (dict(weights={k: v for k, v in w.items() if k != "wl"}, n_members=M), "weights lack 'wl'"),
        (dict(weights=w, n_members=2), r"weights\['w1'\] has shape"),  # stacked for three members, called for two
        (dict(weights=w, n_members=M, n_channels=4), "has shape"),
        (dict(weights=but("wl", _dev(torch.zeros((M, 4, C * cells + 1)))), n_members=M), r"weights\['wl'\] has shape"),
        (dict(weights=but("b2", _dev(torch.zeros((M, C), dtype=torch.float64))), n_members=M), r"weights\['b2'\] has dtype"),
        (dict(weights=but("wh", torch.zeros((M, C, C, 3, 3))), n_members=M), r"weights\['wh'\] lives on cpu"),
        (dict(weights=but("w2", _dev(torch.zeros((M, C, 3, 3, C)).permute(0, 1, 4, 2, 3))), n_members=M), r"weights\['w2'\] must be contiguous"),
        (dict(weights=but("bl", np.zeros((M, 4), dtype=np.float32)), n_members=M), "must be a torch tensor"),
        (dict(weights=w, n_members=M, out=torch.zeros((M, n), dtype=torch.uint8)), "out lives on cpu"),
        (dict(weights=w, n_members=M, out=_dev(torch.zeros((M, n), dtype=torch.int8))), "out has dtype"),
        (dict(weights=w, n_members=M, out=_dev(torch.zeros((M, n + 1), dtype=torch.uint8))), "out has shape"),
        (dict(weights=w, n_members=M, out=_dev(torch.zeros((n, M), dtype=torch.uint8).t())), "out must be contiguous"),
        (dict(weights=w, n_members=M, out=out, scores_out=torch.zeros((M, n, 4))), "scores_out lives on cpu"),
        (dict(weights=w, n_members=M, out=out, scores_out=_dev(torch.zeros((M, n, 4), dtype=torch.float64))), "scores_out has dtype"),
        (dict(weights=w, n_members=M, out=out, scores_out=_dev(torch.zeros((M, n), dtype=torch.float32))), "scores_out has shape"),
        (dict(weights=w, n_members=M, out=out, scores_out=_dev(torch.zeros((M, n, 8))[:, :, ::2])), "scores_out must be contiguous"),
    ]
    for kwargs, message in cases:
        kwargs.setdefault("n_channels", C)
        with pytest.raises(ValueError, match=message):
            env.convq_act_members_all(**kwargs)
    assert scores.shape == (M, n, 4)
    # (the checks are raises, not asserts: `python -O` leaves them in)
    import inspect

    body = "".join(inspect.getsource(getattr(BatchedGridworldEnv, name)) for name in (  # the two and every helper they delegate to
        "convq_act_members_all", "_member_convq_weights", "_members_all_args", "_convq_weights", "_check"))
    for mark in ("n_members must be in", "weights lack", "has shape"):  # (the checks the cases above met are in what was read)
        assert mark in body
    assert "assert " not in body


# ---- the descriptor's own completeness check ---------------------------------------------------------------------------------------------
def test_every_field_of_the_descriptor_names_a_guard_band_test():
    """tests/test_guard_arena_cpu.py's rule for the pointers its parser cannot see: each field of sgk_members_act_out is a non-const
    pointer the library writes through, and each names at least one existing test of the GPU file that carves it from an arena."""
    fields = _struct_fields("sgk_members_act_out")
    for decl, _ in fields:
        assert "*" in decl and "const" not in decl.split("*")[0].split(), decl
    found = {"sgk_members_act_out.%s" % name for _, name in fields}
    assert found == set(ACT_OUT_COVERED), (sorted(found - set(ACT_OUT_COVERED)), sorted(set(ACT_OUT_COVERED) - found))
    for key, tests in ACT_OUT_COVERED.items():
        assert tests, key
        for t in tests:
            module, _, name = t.rpartition(".")
            owner = importlib.import_module(module)
            assert callable(getattr(owner, name, None)) and name.startswith("test_"), (key, t)
            src = open(owner.__file__).read()
            assert "guard_arena" in src and key.split(".")[1][:-len("_dev")] in src, (key, t)
    # and the parameter itself stays out of the header-wide tables' reach: const, as the header explains
    assert "const sgk_members_act_out *out" in _declared("sgk_convq_act_members_all")


# ---- the population and the command line ----------------------------------------------------------------------------------------------
def test_the_population_has_the_ensemble_and_the_command_line_still_refuses_ppo_cnn():
    pop = S.BatchedPPOCNNPopulation
    assert issubclass(pop, ensemble.EnsembleMixin)
    for name in ("ensemble_act", "evaluate_ensemble"):
        assert callable(getattr(pop, name)) and getattr(pop, name) is getattr(ensemble.EnsembleMixin, name)
    assert pop._ensemble_act_all is not ensemble.EnsembleMixin._ensemble_act_all  # the conv launch, not the MLP's
    assert pop._ensemble_weights is not ensemble.EnsembleMixin._ensemble_weights
    for other in (S.BatchedPPOPopulation, S.BatchedDeepQPopulation):  # the MLP populations keep the default hook
        assert other._ensemble_act_all is ensemble.EnsembleMixin._ensemble_act_all
    assert ensemble.ENSEMBLE_AGENTS == ("ppo-mlp", "deep-q")
    cnn = ["ppo-cnn", "-l", "1e-3", "-r", "2", "-e", "2", "-b", "7"]
    for core, agent in ((["--ensemble-eval"], cnn + ["--members", "3"]), ([], cnn + ["--members", "3", "--ensemble-eval"])):
        args = S.prepare_parser().parse_args(core + ["boat"] + agent)
        with pytest.raises(SystemExit, match="ppo-mlp or deep-q agents, not 'ppo-cnn'"):
            ensemble.check_ensemble_eval(args)


def test_the_hook_is_what_the_mixin_calls():
    """ensemble_act goes through _ensemble_act_all with _ensemble_weights() and the [M, N] buffer, then votes over that buffer."""
    calls = []

    class Env:
        n_envs, device = 6, 0

        def members_vote(self, member_actions, members=None, out=None, votes_out=None, dissent=None):
            calls.append(("vote", member_actions, members, out, votes_out))
            return "voted"

        def policy_act_members_all(self, weights, n_members, out=None, scores_out=None):
            calls.append(("mlp", weights, n_members, out))

    class Pop(ensemble.EnsembleMixin):
        n_members, device = 2, "cpu"

        def __init__(self):
            self.env = Env()

        def _ensemble_weights(self):
            return "weights"

    class ConvPop(Pop):
        def _ensemble_act_all(self, weights, out):
            calls.append(("conv", weights, out))

    for cls, kind in ((Pop, "mlp"), (ConvPop, "conv")):
        del calls[:]
        p = cls()
        assert p.ensemble_act(out="o", votes_out="v") == "voted"
        ma = p._ens["member_actions"]
        assert tuple(ma.shape) == (2, 6) and ma.dtype == torch.uint8
        assert calls[0] == ((kind, "weights", 2, ma) if kind == "mlp" else (kind, "weights", ma))
        assert calls[1][0] == "vote" and calls[1][1] is ma and calls[1][2] is None and calls[1][3:] == ("o", "v")
        # (the lockstep step and the graph's warm-up need env.step: tests/test_gpu_convq_ensemble.py)
