"""tests/guard_arena.py on the CPU: what check() must report it reports -- the side, the offset --, what it must not it does not, and
every pointer include/sgk.h lets the library write through is either under a guard-band case of tests/test_gpu_guard_bands.py (COVERED)
or exempt for a stated reason (EXEMPT): a new entry point fails here until somebody decides."""
import importlib
import os
import re

import pytest
import torch

import guard_arena as GA
import test_gpu_guard_bands as GB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arena(pattern="p", nbytes=1 << 18):
    a = GA.Arena("cpu", pattern, nbytes)
    x = a.carve("x", (5, 25), torch.int8, fill=0)                      # 125 bytes, rows of 25: the guard is the 4096-byte minimum
    y = a.carve("y", (3, 2500, 4), torch.float32, fill=0.0)            # a slice of 40 000 bytes: the guard is one slice
    z = a.carve("z", (7,), torch.int64, fill=0, outer=3 * 8)           # a flat tensor with a named outer stride
    return a, x, y, z


@pytest.mark.parametrize("pattern", GA.PATTERNS)
def test_layout(pattern):
    a, x, y, z = _arena(pattern)
    assert a.layout_ok() and a.check() == []
    prev_end = 0
    for name, view, outer in (("x", x, 25), ("y", y, 40000), ("z", z, 24)):
        start, end, guard, outer_bytes = a.span(name)
        assert outer_bytes == outer and guard == max(4096, outer) and guard >= GA.MIN_GUARD
        assert start % 256 == 0 and view.data_ptr() % 256 == 0 and view.is_contiguous()
        assert view.data_ptr() - a.buf.data_ptr() == start and end - start == view.numel() * view.element_size()
        assert start - guard >= prev_end  # its own guard in front, clear of the neighbour's view AND of the neighbour's own guard
        assert end + guard <= a.nbytes
        # nothing but pattern between the views
        lo = prev_end
        assert torch.equal(a.buf[lo:start], GA.pattern_bytes(pattern, lo, start))
        prev_end = end + guard
    assert a.guard_bytes() == a.nbytes - (125 + 3 * 40000 + 56)
    assert a.names() == ["x", "y", "z"]


@pytest.mark.parametrize("pattern", GA.PATTERNS)
def test_a_stray_byte_is_reported_with_its_side_and_offset(pattern):
    for name in ("x", "y", "z"):
        a, *_ = _arena(pattern)
        start, end, guard, outer = a.span(name)
        far = end + max(outer, 1) - 1  # one whole outer slice behind the last one
        for pos, want in ((start - 1, (name, "before", -1, 1)), (end, (name, "after", 0, 1)), (far, (name, "after", far - end, 1)),
                          (start - guard, (name, "before", -guard, 1)), (end + guard - 1, (name, "after", guard - 1, 1))):
            keep = int(a.buf[pos])
            a.buf[pos] = keep ^ 0x01  # one bit
            assert a.check() == [want], (name, pos)
            a.buf[pos] = keep
            assert a.check() == []
    # several at once: every region once, the first offset and the count
    a, *_ = _arena(pattern)
    sx, ex, _, _ = a.span("x")
    a.buf[sx - 3:sx] ^= 0xFF
    a.buf[ex + 5] ^= 0x80
    a.buf[ex + 9] ^= 0x80
    assert a.check() == [("x", "before", -3, 3), ("x", "after", 5, 2)]
    # the allocation's tail behind the last view's guard belongs to that view
    a, *_ = _arena(pattern)
    _, ez, _, _ = a.span("z")
    a.buf[a.nbytes - 1] ^= 0xFF
    assert a.check() == [("z", "after", a.nbytes - 1 - ez, 1)]


@pytest.mark.parametrize("pattern", GA.PATTERNS)
def test_writes_inside_the_views_report_nothing(pattern):
    a, x, y, z = _arena(pattern)
    x.fill_(-1)
    y.fill_(float("nan"))
    z.fill_(-(2 ** 63))
    x[0, 0], x[4, 24], y[0, 0, 0], y[2, 2499, 3], z[0], z[6] = 7, 7, 1.0, 1.0, 3, 3
    assert a.check() == []
    for name in ("x", "y", "z"):
        assert a.unwritten(name) == 0


@pytest.mark.parametrize("pattern", GA.PATTERNS)
def test_a_frozen_input_changed_by_one_bit_is_reported(pattern):
    a, x, y, z = _arena(pattern)
    a.freeze("y")
    x[2, 3] = 9  # an output may change
    assert a.check() == []
    y.view(-1).view(torch.int32)[12345] ^= 1 << 9
    assert a.check() == [("y", "input", 12345 * 4 + 1, 1)]
    y.view(-1).view(torch.int32)[12345] ^= 1 << 9
    assert a.check() == []
    w = a.adopt("w", torch.arange(12, dtype=torch.float32).reshape(3, 4))
    assert w.shape == (3, 4) and w.dtype == torch.float32 and w[2, 3] == 11.0 and w.data_ptr() % 256 == 0
    a.freeze("w")
    w[0, 0] = -0.0  # +0.0 -> -0.0: the sign bit alone
    assert a.check() == [("w", "input", 3, 1)]


def test_unwritten_finds_what_a_call_left_out():
    a = GA.Arena("cpu", "~p", 1 << 16)
    t = a.carve("t", (37,), torch.uint8)  # 9 groups of four and a group of one
    assert a.unwritten("t") == 10
    t[:36] = 2
    assert a.unwritten("t") == 1
    t[36] = 0
    assert a.unwritten("t") == 0
    f = a.carve("f", (6, 4), torch.float32)
    f[:5] = 0.5
    assert a.unwritten("f") == 4


def test_the_two_patterns_differ_at_every_byte():
    p, q = GA.pattern_bytes("p", 0, 70000), GA.pattern_bytes("~p", 0, 70000)
    assert bool((p != q).all()) and bool(((p ^ q) == 0xFF).all())
    assert p[:4].tolist() == [13, 180, 91, 2] and p[255 + 256].item() == (255 * 167 + 13) & 0xFF
    assert sorted(p[:256].tolist()) == list(range(256))  # every byte value occurs: no value is safe from being the pattern somewhere
    a, b = GA.Arena("cpu", "p", 4096), GA.Arena("cpu", "~p", 4096)
    assert torch.equal(a.buf, p[:4096]) and torch.equal(b.buf, q[:4096])
    with pytest.raises(ValueError):
        GA.Arena("cpu", "q")


def test_carving_refuses_an_arena_that_is_too_small():
    a = GA.Arena("cpu", "p", 3 * 4096)
    a.carve("a", (4096,), torch.uint8)  # 4096 + view + 4096: fits exactly
    assert a.layout_ok()
    with pytest.raises(ValueError, match="no room"):
        a.carve("b", (1,), torch.uint8)
    a = GA.Arena("cpu", "p", 3 * 4096)
    with pytest.raises(ValueError, match="no room"):
        a.carve("a", (4097,), torch.uint8)  # one byte more would shorten the guard behind it
    assert a.names() == [] and a.check() == []
    a = GA.Arena("cpu", "p", 1 << 16)
    with pytest.raises(ValueError, match="no room"):
        a.carve("r", (3, 30000), torch.int8)  # the guards are one slice each: 150 000 bytes in all
    a.carve("r", (3, 300), torch.int8)
    with pytest.raises(ValueError, match="twice"):
        a.carve("r", (1,), torch.int8)


# ---- completeness: every pointer the library may write through ---------------------------------------------------------------------------
HANDLES = ("sgk_env", "sgk_tabq", "sgk_comm")  # opaque: `sgk_env *h` is no buffer (`sgk_env **out` is an out-param and is listed)
STRUCTS = ("sgk_dqn_learner", "sgk_ppo_learner", "sgk_ppo_cnn_learner", "sgk_members_explore", "sgk_members_tensor")


def _header():
    text = open(os.path.join(ROOT, "include", "sgk.h")).read()
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _writable(decl, field=False):
    """[name] of the declarators of one parameter / field declaration that are non-const pointers (a parameter: or arrays, which C
    passes as pointers; a struct's `double lo[8]` is a value)."""
    decl = " ".join(decl.split())
    if not decl or decl == "void" or ("*" not in decl and "[" not in decl):
        return []
    base = decl.split("*")[0].split("[")[0].split()
    if "const" in base:
        return []
    if "[" in decl and "*" not in decl:  # int64_t out_host[SGK_METRICS_LEN]
        return [] if field else [re.match(r".*?(\w+)\s*\[", decl).group(1)]
    stars = decl.count("*")
    if base[-1] in HANDLES and stars == 1 and "," not in decl:
        return []
    names = []
    for part in decl[decl.index("*"):].split(","):  # float *w1, *b1, ... / float *m[6], *v[6]
        part = part.strip()
        if part.startswith("*"):
            names.append(re.match(r"\*+\s*(\w+)", part).group(1))
    return names


def header_writable_pointers():
    text = _header()
    found = []
    for m in re.finditer(r"SGK_API\s+[\w\s\*]+?\b(\w+)\s*\(([^)]*)\)\s*;", text):
        fn, params = m.group(1), m.group(2)
        for p in params.split(","):
            found += ["%s.%s" % (fn, n) for n in _writable(p)]
    for s in STRUCTS:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (s, s), text, flags=re.S).group(1)
        for decl in body.split(";"):
            found += ["%s.%s" % (s, n) for n in _writable(decl, field=True)]
    return found


def test_the_parser_sees_what_the_header_says():
    found = header_writable_pointers()
    assert len(found) == len(set(found)) and len(found) > 150
    for k in ("sgk_obs_f32.dst_dev", "sgk_finished.n_host", "sgk_create.out", "sgk_metrics.out_host", "sgk_dqn_learner.vmax",
              "sgk_dqn_learner.w3t", "sgk_dqn_learner.rows_out", "sgk_ppo_learner.stats_out", "sgk_ppo_cnn_learner.workspace",
              "sgk_ppo_cnn_learner.params", "sgk_members_explore.generation_dev", "sgk_step_store.terminals_ring",
              "sgk_dqn_sgd_step_members.workspace", "sgk_debug_host_step.aux_env", "sgk_policy_rollout_members_eps.member_metrics_dev"):
        assert k in found, k
    for k in ("sgk_step.h", "sgk_step.actions_dev", "sgk_dqn_learner.rows", "sgk_dqn_learner.tw1t", "sgk_dqn_sgd_step.learner",
              "sgk_members_vote.member_actions_dev", "sgk_tabq_load_shared.table_dev", "sgk_ppo_cnn_learner.old_params", "sgk_members_explore.lo"):
        assert k not in found, k


def test_every_writable_pointer_is_covered_or_exempt():
    found = set(header_writable_pointers())
    covered, exempt = set(GB.COVERED), set(GB.EXEMPT)
    assert not covered & exempt, sorted(covered & exempt)
    undecided = sorted(found - covered - exempt)
    assert not undecided, "no guard-band case and no exemption for: %s" % ", ".join(undecided)
    stale = sorted((covered | exempt) - found)
    assert not stale, "not (or no longer) a writable pointer of include/sgk.h: %s" % ", ".join(stale)
    for k, reason in GB.EXEMPT.items():
        assert isinstance(reason, str) and len(reason.strip()) >= 8 and "\n" not in reason, k
    for k, tests in GB.COVERED.items():
        assert tests, k
        for t in tests:  # a test of the guard-band file, or "module.test" of another file of the suite
            module, _, name = t.rpartition(".")
            owner = importlib.import_module(module) if module else GB
            assert callable(getattr(owner, name, None)) and name.startswith("test_"), (k, t)
