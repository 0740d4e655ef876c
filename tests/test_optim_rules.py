"""-optim / -optim_cnn sgd and rmsprop (reference utils/utils.py:78-87, train.py:239-240) on the fused flat steps: which optimizer
train.build_optimizers builds, that the gradient exchange covers their groups, and their state_dicts (own format, torch.optim's,
another rule's).  CPU only: no kernel is launched."""
import pytest
import torch

from helpers import mk_args


def _args(optim="adam", optim_cnn="adam", **kw):
    return mk_args(hidden_size=32, maxseqlen=3, lr=1e-3, lr_cnn=1e-5, weight_decay=1e-6, weight_decay_cnn=1e-6, optim=optim,
                   optim_cnn=optim_cnn, momentum=0.9, **kw)


def _models(a):
    from rsis_amd.modules import FeatureExtractor, RSIS
    torch.manual_seed(0)
    return FeatureExtractor(a), RSIS(a)


@pytest.mark.parametrize("optim,optim_cnn", [("sgd", "rmsprop"), ("rmsprop", "sgd"), ("adam", "sgd"), ("sgd", "adam")])
def test_build_optimizers_picks_the_rule_per_group(optim, optim_cnn):
    from rsis_amd.optim import FlatAdam, FlatRMSprop, FlatSGD
    from rsis_amd.train import build_optimizers
    cls = {"adam": FlatAdam, "sgd": FlatSGD, "rmsprop": FlatRMSprop}
    a = _args(optim, optim_cnn, use_class_loss=False, use_stop_loss=False)
    enc, dec = _models(a)
    enc_opt, dec_opt = build_optimizers(a, enc, dec)
    assert type(dec_opt) is cls[optim] and type(enc_opt) is cls[optim_cnn]
    assert dec_opt.group.lr == a.lr and enc_opt.group.lr == a.lr_cnn
    # the heads whose losses are off start inactive under every rule
    heads = set(id(p) for p in list(dec.fc_class.parameters()) + list(dec.fc_stop.parameters()))
    g = dec_opt.group
    assert [not act for act in g.active] == [id(p) in heads for p in g.params]
    for o in (enc_opt, dec_opt):
        if type(o) is not FlatAdam:
            # one state buffer, none of Adam's moments
            assert not hasattr(o.group, "exp_avg") and o.group.buf.numel() == o.group.flat_p.numel()
    if optim == "sgd":
        assert dec_opt.group.hyper == {"momentum": 0.9}


def test_build_optimizers_honours_momentum():
    from rsis_amd.train import build_optimizers
    a = _args("sgd", "sgd")
    a.momentum = 0.5
    enc, dec = _models(a)
    enc_opt, dec_opt = build_optimizers(a, enc, dec)
    assert enc_opt.group.hyper["momentum"] == dec_opt.group.hyper["momentum"] == 0.5


def test_enc_lr_quirk_needs_adam():
    from rsis_amd.train import build_optimizers
    a = _args("adam", "sgd", enc_lr_quirk=True)
    enc, dec = _models(a)
    with pytest.raises(Exception, match="enc_lr_quirk"):
        build_optimizers(a, enc, dec)


def _spans(plan, groups):
    out = {}
    for stage, views in plan.items():
        spans = []
        for t in views:
            k = next(i for i, g in enumerate(groups) if t.untyped_storage().data_ptr() == g.flat_g.untyped_storage().data_ptr())
            spans.append((k, t.storage_offset(), t.numel()))
        out[stage] = spans
    return out


@pytest.mark.parametrize("rule", ["sgd", "rmsprop"])
def test_exchange_plan_covers_every_rule(rule):
    """the staged gradient exchange must all-reduce the decoder group whatever its rule: with an empty "dec" list the replicas would
    drift apart without an error at world > 1"""
    from rsis_amd.train import build_optimizers, exchange_plan
    plans = []
    for optim in ("adam", rule):
        a = _args(optim, optim)
        enc, dec = _models(a)
        enc_opt, dec_opt = build_optimizers(a, enc, dec)
        for cuts in (0, 1, 2):
            plans.append((optim, cuts, _spans(exchange_plan(enc, [enc_opt, dec_opt], cuts), [enc_opt.group, dec_opt.group])))
    adam, other = plans[:3], plans[3:]
    for (_, c1, p1), (_, c2, p2) in zip(adam, other):
        assert c1 == c2 and p1 == p2
        assert sum(n for _k, _o, n in p2["dec"] + p2["trunk_hi"] + p2["rest"]) > 0
    assert other[1][2]["dec"] == [(1, 0, dec_opt.group.flat_g.numel())]


def _torch_state(rule, n_steps=3):
    """a torch.optim state_dict after n_steps CPU steps; the second of three parameters never gets a gradient"""
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(torch.randn(s)) for s in ((4, 3), (5,), (2, 3, 2))]
    opt = (torch.optim.SGD(ps, lr=1e-2, momentum=0.9, weight_decay=1e-2) if rule == "sgd"
           else torch.optim.RMSprop(ps, lr=1e-2, weight_decay=1e-2))
    for _ in range(n_steps):
        opt.zero_grad(set_to_none=True)
        (ps[0].square().sum() + ps[2].sin().sum()).backward()
        opt.step()
    return ps, opt.state_dict()


def _flat(rule, ps, **kw):
    from rsis_amd.optim import FlatRMSprop, FlatSGD
    fresh = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    return (FlatSGD if rule == "sgd" else FlatRMSprop)(fresh, lr=1e-2, **kw)


@pytest.mark.parametrize("rule", ["sgd", "rmsprop"])
def test_torch_state_dict_is_adopted(rule):
    key = {"sgd": "momentum_buffer", "rmsprop": "square_avg"}[rule]
    ps, sd = _torch_state(rule)
    opt = _flat(rule, ps)
    assert opt.load_state_dict(sd) is True
    g = opt.group
    ids = sd["param_groups"][0]["params"]
    for k, (i, (off, n)) in enumerate(zip(ids, g.offsets)):
        if i in sd["state"]:
            assert torch.equal(g.buf[off:off + n], sd["state"][i][key].reshape(-1)), k
            assert g.active[k]
        else:                                  # no gradient yet: inactive, zero buffer
            assert not g.active[k] and float(g.buf[off:off + n].abs().sum()) == 0.0
    assert g.active == [True, False, True]
    assert [r[3] for r in g.ranges()] == [[0], [2]]


@pytest.mark.parametrize("rule", ["sgd", "rmsprop"])
def test_state_dicts_that_do_not_fit_are_refused(rule):
    from rsis_amd.optim import FlatAdam
    ps, sd = _torch_state(rule)
    # a parameter list that does not line up: False, zeros, no exception
    opt = _flat(rule, ps[:2])
    assert opt.load_state_dict(sd) is False
    assert float(opt.group.buf.abs().sum()) == 0.0 and all(opt.group.active)
    # Adam state into this rule, both forms
    _, adam_sd = _torch_state_adam(ps)
    opt = _flat(rule, ps)
    assert opt.load_state_dict(adam_sd) is False
    adam = FlatAdam([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=1e-2)
    adam.group.exp_avg.normal_()
    assert opt.load_state_dict(adam.state_dict()) is False
    assert float(opt.group.buf.abs().sum()) == 0.0
    # this rule's state into Adam, both forms: False, no KeyError
    adam = FlatAdam([torch.nn.Parameter(p.detach().clone()) for p in ps], lr=1e-2)
    assert adam.load_state_dict(sd) is False
    mine = _flat(rule, ps)
    mine.group.buf.normal_()
    assert adam.load_state_dict(mine.state_dict()) is False
    assert float(adam.group.exp_avg.abs().sum()) == 0.0 and adam.group.steps == [0, 0, 0]
    # the other flat rule's own state
    other = _flat("rmsprop" if rule == "sgd" else "sgd", ps)
    assert opt.load_state_dict(other.state_dict()) is False


def _torch_state_adam(ps):
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt = torch.optim.Adam(qs, lr=1e-3)
    qs[0].grad = torch.ones_like(qs[0])
    opt.step()
    return qs, opt.state_dict()


@pytest.mark.parametrize("rule", ["sgd", "rmsprop"])
def test_own_checkpoint_roundtrip(tmp_path, rule):
    from rsis_amd.args import get_parser
    from rsis_amd.modules import RSIS, FeatureExtractor
    from rsis_amd.train import build_optimizers
    from rsis_amd.utils.utils import load_checkpoint, save_checkpoint
    a = get_parser().parse_args(["-model_name", "own", "-hidden_size", "32", "-num_classes", "7", "-optim", rule, "-optim_cnn", rule,
                                 "-momentum", "0.8"])
    a.models_root = str(tmp_path)
    a.use_gpu = False
    torch.manual_seed(0)
    enc, dec = FeatureExtractor(a), RSIS(a)
    enc_opt, dec_opt = build_optimizers(a, enc, dec)
    enc_opt.group.buf.uniform_()
    dec_opt.group.buf.uniform_()
    dec_opt.group.active[-1] = False
    save_checkpoint(a, enc, dec, enc_opt, dec_opt, root=str(tmp_path))
    e_sd, d_sd, e_o, d_o, largs = load_checkpoint("own", use_gpu=False, root=str(tmp_path))
    assert largs.optim == rule and e_o["optim"] == d_o["optim"] == rule
    if rule == "sgd":
        assert d_o["momentum"] == pytest.approx(0.8)
    enc2, dec2 = FeatureExtractor(largs), RSIS(largs)
    enc2.load_state_dict(e_sd)
    dec2.load_state_dict(d_sd)
    enc_opt2, dec_opt2 = build_optimizers(largs, enc2, dec2)
    assert enc_opt2.load_state_dict(e_o) is True and dec_opt2.load_state_dict(d_o) is True
    assert torch.equal(enc_opt2.group.buf, enc_opt.group.buf) and torch.equal(dec_opt2.group.buf, dec_opt.group.buf)
    assert dec_opt2.group.active == dec_opt.group.active
