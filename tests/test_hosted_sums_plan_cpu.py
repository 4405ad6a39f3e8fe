"""The backward epilogue's launch plan with a queued grad-h launch (``launch_group.plan`` / ``flush``), no GPU: which queued
jobs the grad-h launch carries, which stay for the launch behind it, that the sum of grad-h's own partials is never carried,
and that without a queued grad-h launch (``QOT_NO_HOSTED_SUMS=1``, or a pass without an H = 64 NNConv) the plan is the
two-stage one.  ``_lib``'s launching functions are replaced by recorders; the role records are the real ctypes ones."""
import ctypes

import pytest
import torch

from gnn_qot_estimation_amd import _lib, launch_group as LG


def role(kind, tag):
    return _lib.make_role(kind, (tag,), (tag,))        # tag: told apart by p[0] / i[0]


def tags(roles):
    return [(r.kind, r.i[0]) for r in roles]


SUM, SLAB, GHSUM, FIN = _lib.ROLE_SUM_ROWS, _lib.ROLE_NNCONV_SLAB_SUM64, _lib.ROLE_NNCONV_GRADH_SUM64, _lib.ROLE_NNCONV_FINALIZE64
BWD = _lib.ROLE_TABLE_PROJECT_BWD_SCORES


def test_role_numbers_match_the_header():
    hdr = open(__import__("os").path.join(__import__("os").path.dirname(_lib.__file__), "..", "include", "qot_gnn.h")).read()
    assert f"QOT_ROLE_NNCONV_SLAB_SUM64 = {SLAB}" in hdr and f"QOT_ROLE_NNCONV_GRADH_SUM64 = {GHSUM}" in hdr
    assert "QOT_ROLE_NNCONV_FINALIZE64 = 5" in hdr and FIN == 5
    assert "int qot_nnconv_gradh_host_roles(const qot_role_t* roles, int n_roles);" in hdr
    assert set(_lib.HOSTABLE_ROLES) == {SUM, SLAB}


def test_grad_h_carries_every_stage_one_sum_and_its_own_sum_rides_with_stage_two():
    # the flagship step's queue: read-out partials, loss rows, slab sum, TransformerConv row sum | table projection backward
    s1 = [role(SUM, 1), role(SUM, 2), role(SLAB, 3), role(SUM, 4)]
    s2 = [role(BWD, 5)]
    gh = role(GHSUM, 6)
    steps = LG.plan(s1, s2, [("qot_nnconv_gradh_split", (7,), gh)])
    assert [s[0] for s in steps] == ["gradh", "roles"]
    assert steps[0][1:3] == ("qot_nnconv_gradh_split", (7,)) and tags(steps[0][3]) == [(SUM, 1), (SUM, 2), (SLAB, 3), (SUM, 4)]
    assert tags(steps[1][1]) == [(BWD, 5), (GHSUM, 6)]


def test_the_sum_of_grad_h_partials_is_never_carried_and_other_kinds_keep_their_launch():
    # a full finalize role (reads grad-h's partials), a grad-h sum of another layer and a heavy kind queued in stage 1
    s1 = [role(FIN, 1), role(SUM, 2), role(GHSUM, 3), role(BWD, 4)]
    steps = LG.plan(s1, [role(BWD, 5)], [("f", (), role(GHSUM, 6))])
    assert [s[0] for s in steps] == ["gradh", "roles", "roles"]
    assert tags(steps[0][3]) == [(SUM, 2)]
    assert tags(steps[1][1]) == [(FIN, 1), (GHSUM, 3), (BWD, 4), (GHSUM, 6)]      # stage 1's rest, in front of stage 2
    assert tags(steps[2][1]) == [(BWD, 5)]
    for s in steps:
        if s[0] == "gradh":
            assert all(r.kind in _lib.HOSTABLE_ROLES for r in s[3])


def test_more_sums_than_a_table_holds_stay_behind_and_a_second_grad_h_launch_carries_nothing():
    s1 = [role(SUM, k) for k in range(_lib.MAX_ROLES + 3)]
    steps = LG.plan(s1, [], [("f", (1,), role(GHSUM, 100)), ("f", (2,), role(GHSUM, 101))])
    assert [s[0] for s in steps] == ["gradh", "gradh", "roles"]
    assert tags(steps[0][3]) == [(SUM, k) for k in range(_lib.MAX_ROLES)] and steps[1][3] == []
    assert tags(steps[2][1]) == [(SUM, _lib.MAX_ROLES + k) for k in range(3)] + [(GHSUM, 100), (GHSUM, 101)]


def test_a_queue_without_a_deferred_grad_h_launch_plans_as_before():
    s1, s2 = [role(SUM, 1), role(FIN, 2)], [role(BWD, 3)]
    steps = LG.plan(s1, s2, [])
    assert [s[0] for s in steps] == ["roles", "roles"] and steps[0][1] is s1 and steps[1][1] is s2
    assert LG.plan(s1, [], []) == [("roles", s1)] and LG.plan([], [], []) == []


class Recorder:
    """Stands in for ``launch_group._lib``: records what would be launched, in order."""
    MAX_ROLES, HOSTABLE_ROLES, make_role = _lib.MAX_ROLES, _lib.HOSTABLE_ROLES, staticmethod(_lib.make_role)

    def __init__(self):
        self.log, self.pinned = [], None

    def stream(self):
        return 1234

    def on_stream(self, handle):
        rec = self

        class Pin:
            def __enter__(self):
                rec.pinned = handle

            def __exit__(self, *exc):
                rec.pinned = None
        return Pin()

    def host_roles(self, roles):
        self.log.append(("host", tags(roles)))

    def call(self, name, *args):
        self.log.append(("call", name, args, self.pinned))

    def run_roles(self, roles, stream_handle=None):
        if roles:
            self.log.append(("roles", tags(roles), stream_handle))


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(LG, "_lib", r)
    monkeypatch.setattr(LG, "_arm", lambda: (LG._Q.__setattr__("stream", 1234), LG._Q)[1])     # no autograd engine here
    monkeypatch.delenv("QOT_NO_LAUNCH_GROUPS", raising=False)
    monkeypatch.delenv("QOT_NO_HOSTED_SUMS", raising=False)
    monkeypatch.delenv("QOT_HOSTED_SUMS_EARLY", raising=False)
    LG._Q.clear()
    yield r
    LG._Q.clear()


def test_flush_launches_grad_h_on_the_queue_stream_with_its_hosted_sums_first(rec):
    keep = torch.zeros(1)
    LG.defer(SUM, (1,), (1,), stage=1)
    LG.defer(SLAB, (2,), (2,), stage=1)
    LG.defer_gradh("qot_nnconv_gradh_split", (11, 12), (GHSUM, (3,), (3,)), keep=(keep,))
    LG.defer(SUM, (4,), (4,), stage=1)                       # queued AFTER grad-h (TransformerConv's row sum): carried too
    LG.defer(BWD, (5,), (5,), stage=2)
    assert LG._Q.pending() and rec.log == []                 # nothing is launched before the flush
    LG.flush()
    assert rec.log == [("host", [(SUM, 1), (SLAB, 2), (SUM, 4)]), ("call", "qot_nnconv_gradh_split", (11, 12), 1234),
                       ("roles", [(BWD, 5), (GHSUM, 3)], 1234)]
    assert not LG._Q.pending() and LG._Q.keep == [] and LG._Q.gradh == []


def test_a_queued_grad_h_launch_alone_is_pending_and_flushed(rec):
    LG.defer_gradh("f", (1,), (GHSUM, (3,), (3,)))
    assert LG._Q.pending()
    LG.flush()
    assert rec.log == [("call", "f", (1,), 1234), ("roles", [(GHSUM, 3)], 1234)]          # nothing to host: no host call
    LG._Q.gradh.append(("f", (), role(GHSUM, 1)))
    LG._Q.armed = True
    LG.drop_stale()
    assert not LG._Q.pending()


def test_early_mode_launches_grad_h_at_once_with_what_is_queued_by_then(rec, monkeypatch):
    monkeypatch.setenv("QOT_HOSTED_SUMS_EARLY", "1")
    LG.defer(SUM, (1,), (1,), stage=1)
    LG.defer(BWD, (9,), (9,), stage=1)
    LG.defer_gradh("f", (7,), (GHSUM, (3,), (3,)))
    assert rec.log == [("host", [(SUM, 1)]), ("call", "f", (7,), 1234)]
    LG.defer(SUM, (4,), (4,), stage=1)
    LG.flush()
    assert rec.log[2:] == [("roles", [(BWD, 9), (GHSUM, 3), (SUM, 4)], 1234)]


def test_the_switch_is_read_on_every_call(monkeypatch):
    monkeypatch.delenv("QOT_NO_HOSTED_SUMS", raising=False)
    assert LG.hosted_sums()
    monkeypatch.setenv("QOT_NO_HOSTED_SUMS", "1")
    assert not LG.hosted_sums()
    monkeypatch.setenv("QOT_NO_HOSTED_SUMS", "0")
    assert LG.hosted_sums()


def test_host_roles_refuses_bad_tables_without_a_gpu_and_stores_nothing():
    lib = _lib.load()
    ok = lambda *roles: (_lib.Role * len(roles))(*roles)
    assert lib.qot_nnconv_gradh_host_roles(None, 0) == 0
    assert lib.qot_nnconv_gradh_host_roles(None, 1) < 0                                       # null table
    arr = ok(_lib.make_role(_lib.ROLE_SUM_ROWS, (16, 32), (4, 4, 0)))
    assert lib.qot_nnconv_gradh_host_roles(ctypes.addressof(arr), _lib.MAX_ROLES + 1) < 0     # too many
    for kind in (FIN, GHSUM, BWD, _lib.ROLE_GATHER3, _lib.ROLE_CSR_BY_GRAPH):
        arr = ok(_lib.make_role(kind, tuple(range(16, 16 + 18)), (4, 1, 4, 4)))
        assert lib.qot_nnconv_gradh_host_roles(ctypes.addressof(arr), 1) == -1, kind           # QOT_ERR_UNSUPPORTED: heavy kinds
    arr = ok(_lib.make_role(99, (), ()))
    assert lib.qot_nnconv_gradh_host_roles(ctypes.addressof(arr), 1) == -2                    # unknown kind
    arr = ok(_lib.make_role(_lib.ROLE_SUM_ROWS, (None, None), (4, 4, 0)))
    assert lib.qot_nnconv_gradh_host_roles(ctypes.addressof(arr), 1) == -2                    # NULL operands
    arr = ok(_lib.make_role(SLAB, (16, None, None), (64, 1)))
    assert lib.qot_nnconv_gradh_host_roles(ctypes.addressof(arr), 1) == -2                    # slab sum without a destination
    assert lib.qot_nnconv_gradh_host_roles(None, 0) == 0                                      # (leave nothing behind)
