"""The step route (model_base.StepRoute: what one method of a forward / backward pass tells a later method of the same pass)
is not inherited from a step that failed midway, nor from the step before by an entry that stages a batch of its own.  On
the CPU through the mock backend behind test_host_step_tail's recorder."""
import copy

import pytest

from masters_thesis_amd.model_base import StepRoute
from test_host_step_tail import Injected, make, batch, trace, mock_backend       # noqa: F401 (mock_backend: autouse fixture)

SWITCHES = [{}, {"fused_update": False}, {"sparse_emb_bwd": False}]


def routes_after_staging(model):
    """the route record as every later _stage_batch of ``model`` leaves it: the state in which the step's pass begins"""
    seen, stage = [], model._stage_batch

    def spy(*a, **k):
        out = stage(*a, **k)
        seen.append(copy.copy(model._route))
        return out
    model._stage_batch = spy
    return seen


@pytest.mark.parametrize("switch", SWITCHES, ids=["same step", "fused_update off behind the failure",
                                                  "sparse_emb_bwd off behind the failure"])
@pytest.mark.parametrize("kind,fail_on", [("dense", "lstm_step_bwd"), ("attention", "attention_step_bwd"),
                                          ("attention", "embedding_bwd_sparse")])
def test_a_step_that_failed_in_its_backward_leaves_nothing_to_the_next_steps(kind, fail_on, switch, mock_backend):
    """A fused step raises inside its backward, between the method that parks a hand-off and the one that takes it: the
    dense model behind _bwd_head (the head-bias column sums wait for _bwd_seq_lstm), the attention model inside its chain
    (behind _bwd_head's dout_masked) and in its Embedding backward (behind the chain's dtext_done / dw2_done).  The next
    train_step and the next test_step issue exactly the calls of a model whose step did not fail, and their passes begin
    on the empty record.  (dense, lstm_step_bwd, fused_update off): the commit before StepRoute issued one colsum2 more,
    from the column sums the failed step had parked."""
    be = mock_backend
    fresh = make(kind)
    fresh.train_step(batch(3)).as_floats()
    want = trace(be, fresh, switch)

    model = make(kind)
    model.train_step(batch(3)).as_floats()
    del be.calls[:]
    be.fail_on = fail_on
    with pytest.raises(Injected):
        model.train_step(batch(6))
    assert be.fail_on is None and not any(c.startswith(("step_finalize(", "adam(", "adam_fin(")) for c in be.calls)
    seen = routes_after_staging(model)
    assert trace(be, model, switch) == want
    assert seen == [StepRoute(), StepRoute()]


def test_entries_behind_a_step_that_staged_its_masks_generate_their_own(mock_backend):
    """train_step stages the stored attention keep-masks with its batch (route.masks_staged).  A test_step and a
    call_attention(training=True) directly behind it issue the calls of a model that never trained: the training forward of
    call_attention generates the masks itself."""
    be = mock_backend
    runs = []
    for trained in (False, True):
        model = make("attention", attn_units=8, dropout_attn=0.25)
        if trained:
            seen = routes_after_staging(model)
            model.train_step(batch(3)).as_floats()
            assert seen == [StepRoute(masks_staged=True)] and any(c.startswith("dropout_mask4(") for c in be.calls)
        else:
            model._build(*batch(3)[0][1].shape)          # the buffers and the optimizer state, without a step
        out = []
        for entry in (lambda: model.test_step(batch(5)).as_floats(), lambda: model.call_attention(batch(7)[0], training=True)):
            del be.calls[:]
            entry()
            out.append(list(be.calls))
            assert model._route.masks_staged is False
        runs.append(out)
    assert runs[0] == runs[1]
    assert not any(c.startswith("dropout_mask4(") for c in runs[1][0])          # test_step: no Dropout, no masks
    assert sum(c.startswith("dropout_mask4(") for c in runs[1][1]) == 1
