"""derived.py, the one cache of tensors made from a module's parameters and buffers: its key (version, pointer), `invalidate`, the
eval-BatchNorm fold and the predicate for what it folds.  CPU only."""
import pytest
import torch
from torch import nn

from srfdet3d_amd import derived, nhwc


def _counting(fn):
    calls = []

    def make():
        calls.append(1)
        return fn()
    return make, calls


def test_get_builds_once_and_follows_version_and_pointer():
    lin = nn.Linear(3, 2)
    make, calls = _counting(lambda: lin.weight.detach() * 2)
    a = derived.get(lin, "twice", (lin.weight,), make)
    assert derived.get(lin, "twice", (lin.weight,), make) is a and len(calls) == 1
    assert not a.requires_grad and derived.names(lin) == {"twice"}
    with torch.no_grad():
        lin.weight.add_(1.0)                                      # version bump
    b = derived.get(lin, "twice", (lin.weight,), make)
    assert len(calls) == 2 and torch.equal(b, lin.weight.detach() * 2)
    lin.weight.data = torch.ones(2, 3)                            # pointer change, same version
    c = derived.get(lin, "twice", (lin.weight,), make)
    assert len(calls) == 3 and torch.equal(c, torch.full((2, 3), 2.0))
    assert derived.get(lin, "twice", (lin.weight,), make) is c and len(calls) == 3


def test_get_runs_make_without_grad():
    lin = nn.Linear(3, 2)
    with torch.enable_grad():
        assert not derived.get(lin, "sq", (lin.weight,), lambda: lin.weight * lin.weight).requires_grad


def test_a_none_result_is_cached():
    lin = nn.Linear(3, 2)
    make, calls = _counting(lambda: None)
    assert derived.get(lin, "nothing", (lin.weight,), make) is None
    assert derived.get(lin, "nothing", (lin.weight,), make) is None
    assert len(calls) == 1 and derived.names(lin) == {"nothing"}


def test_invalidate_drops_everything_of_every_module():
    inner = nn.Sequential(nn.Linear(3, 3), nn.BatchNorm1d(3).eval())
    model = nn.Sequential(inner, nn.Linear(3, 2), nn.ReLU())
    held = [inner[0], inner[1], model[1]]
    for m in held:
        for name in ("a", "b", "c"):
            derived.get(m, name, (m.weight,), lambda: m.weight.detach().clone())
        assert derived.names(m) == {"a", "b", "c"}
    before = {id(m): dict(m.__dict__) for m in (model, inner, model[2])}
    derived.invalidate(model)
    for m in model.modules():
        assert "_srf_derived" not in m.__dict__ and derived.names(m) == set()
    for m in (model, inner, model[2]):                            # never held anything: untouched
        assert m.__dict__ == before[id(m)]
    assert "_srf_derived" not in model.state_dict() and len(model.state_dict()) == 9


def _random_bn(cls, seed):
    torch.manual_seed(seed)
    bn = cls(24, eps=1e-3).eval()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
        bn.running_mean.normal_(0, 0.1)
        bn.running_var.uniform_(0.5, 1.5)
    return bn


def _fold_by_definition(bn):
    with torch.no_grad():
        scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        return scale, bn.bias - bn.running_mean * scale


@pytest.mark.parametrize("cls", [nn.BatchNorm1d, nn.BatchNorm2d])
def test_fold_bn_is_the_definition_and_cached(cls):
    bn = _random_bn(cls, 1)
    scale, shift = derived.fold_bn(bn)
    want = _fold_by_definition(bn)
    assert torch.equal(scale, want[0]) and torch.equal(shift, want[1])
    assert scale.is_contiguous() and shift.is_contiguous() and not scale.requires_grad
    again = derived.fold_bn(bn)
    assert again[0].data_ptr() == scale.data_ptr() and again[1].data_ptr() == shift.data_ptr()
    for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var):      # keyed on all four
        with torch.no_grad():
            t.mul_(1.5)
        got, want = derived.fold_bn(bn), _fold_by_definition(bn)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("cls", [nn.BatchNorm1d, nn.BatchNorm2d])
def test_invalidate_caches_reaches_the_batchnorm_fold(cls):
    """An update through `.data` is invisible to the key; nhwc.invalidate_caches is what makes the next fold see it."""
    bn = _random_bn(cls, 2)
    old = derived.fold_bn(bn)
    bn.weight.data.mul_(2.0)
    stale = derived.fold_bn(bn)
    assert stale[0] is old[0] and stale[1] is old[1]
    nhwc.invalidate_caches(nn.Sequential(bn))
    got, want = derived.fold_bn(bn), _fold_by_definition(bn)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], old[0])


@pytest.mark.parametrize("cls,other", [(nn.BatchNorm1d, nn.BatchNorm2d), (nn.BatchNorm2d, nn.BatchNorm1d)])
def test_foldable_bn_is_an_eval_mode_affine_batchnorm_of_the_class_asked_for(cls, other):
    assert derived.foldable_bn(cls(8).eval(), cls)
    assert not derived.foldable_bn(cls(8).eval(), other)
    assert not derived.foldable_bn(cls(8).train(), cls)
    assert not derived.foldable_bn(cls(8, affine=False).eval(), cls)
    assert not derived.foldable_bn(cls(8, track_running_stats=False).eval(), cls)
    assert not derived.foldable_bn(nn.GroupNorm(2, 8).eval(), cls) and not derived.foldable_bn(None, cls)


def test_the_two_names_over_foldable_bn():
    from srfdet3d_amd import dense, sparse
    assert dense._foldable(nn.BatchNorm2d(8).eval()) and not dense._foldable(nn.BatchNorm1d(8).eval())
    assert sparse._bn_foldable(nn.BatchNorm1d(8).eval()) and not sparse._bn_foldable(nn.BatchNorm2d(8).eval())
    assert not dense._foldable(nn.BatchNorm2d(8)) and not sparse._bn_foldable(nn.BatchNorm1d(8))
