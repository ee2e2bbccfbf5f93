"""EMA of the weights, the parts that need no GPU: the package's `training_utils.EMA` against the reference's class (where the
reference tree is present) and against the numpy restatement tests/ema_ref.py (everywhere), its CPU API, the model-directory round
trip, and the C ABI surface of the feature."""
import importlib.util
import inspect
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import ema_ref
import util

REF = "/root/reference"
needs_reference = pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is only present in the build container")

NEW_ENTRY_POINTS = ("showo_ema_table_create", "showo_ema_table_update", "showo_ema_table_swap", "showo_ema_table_destroy",
                    "showo_train_bind_ema", "showo_train_set_ema", "showo_train_ema_swap")
STATE_KEYS = ["decay", "min_decay", "optimization_step", "update_after_step", "use_ema_warmup", "inv_gamma", "power", "shadow_params"]
METHODS = ["get_decay", "step", "copy_to", "to", "state_dict", "store", "restore", "load_state_dict", "save_pretrained", "from_pretrained"]
DECAY_STEPS = list(range(13)) + [100, 31623, 10 ** 6]
SCHEDULES = [dict(use_ema_warmup=w, update_after_step=u, min_decay=m) for w in (False, True) for u in (0, 3) for m in (0.0, 0.5)]
SHAPES = [(1,), (257,), (3, 5), (4,)]  # the last one does not require grad


def EMA():
    return util.pkg().training_utils.EMA


_REF_EMA = []


def _reference_ema():
    """the reference's class, loaded from its file alone (the module imports pandas, which it does not use for the EMA)"""
    if _REF_EMA:
        return _REF_EMA[0]
    stubbed = False
    try:
        import pandas  # noqa: F401
    except Exception:
        sys.modules["pandas"] = types.ModuleType("pandas")
        stubbed = True
    try:
        spec = importlib.util.spec_from_file_location("ref_models_training_utils", os.path.join(REF, "models", "training_utils.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if stubbed:
            del sys.modules["pandas"]
    _REF_EMA.append(mod.EMA)
    return mod.EMA


def _tensors(seed=0):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(*s, generator=g) for s in SHAPES]
    for p in ps[:-1]:
        p.requires_grad_(True)
    return ps


def _nudge(ps, g):
    """move every parameter a little (the frozen one too: its shadow must follow by copy)"""
    with torch.no_grad():
        for p in ps:
            p.add_(0.01 * torch.randn(p.shape, generator=g))


# ---------------------------------------------------------------- against the reference

@needs_reference
def test_surface_matches_the_reference_class():
    R, P = _reference_ema(), EMA()
    rs, ps = inspect.signature(R.__init__).parameters, inspect.signature(P.__init__).parameters
    assert list(rs) == list(ps)
    for k in rs:
        assert rs[k].default == ps[k].default and rs[k].kind == ps[k].kind, k
    for m in METHODS:
        assert callable(getattr(R, m)) and callable(getattr(P, m)), m
        if m != "from_pretrained":
            assert list(inspect.signature(getattr(R, m)).parameters) == list(inspect.signature(getattr(P, m)).parameters), m
    assert list(inspect.signature(R.from_pretrained).parameters) == list(inspect.signature(P.from_pretrained).parameters)
    r, p = R(_tensors()), P(_tensors())
    assert list(r.state_dict()) == list(p.state_dict()) == STATE_KEYS
    for attr in ("shadow_params", "temp_stored_params", "optimization_step", "cur_decay_value"):
        assert hasattr(r, attr) and hasattr(p, attr), attr
    assert p.temp_stored_params is None and p.optimization_step == 0 and p.cur_decay_value is None


@needs_reference
@pytest.mark.parametrize("kw", SCHEDULES)
def test_get_decay_matches_the_reference(kw):
    r, p = _reference_ema()(_tensors(), decay=0.9999, **kw), EMA()(_tensors(), decay=0.9999, **kw)
    for t in DECAY_STEPS:
        assert r.get_decay(t) == p.get_decay(t), (kw, t)


@needs_reference
def test_six_cpu_steps_match_the_reference_bit_for_bit():
    kw = dict(decay=0.999, use_ema_warmup=True, update_after_step=1)
    pr, pp = _tensors(3), _tensors(3)
    r, p = _reference_ema()(pr, **kw), EMA()(pp, **kw)
    gr, gp = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    for _ in range(6):
        _nudge(pr, gr)
        _nudge(pp, gp)
        r.step(pr)
        p.step(pp)
        assert r.optimization_step == p.optimization_step and r.cur_decay_value == p.cur_decay_value
        for i, (x, y) in enumerate(zip(r.shadow_params, p.shadow_params)):
            assert torch.equal(x, y), i
    assert p.optimization_step == 6 and torch.equal(p.shadow_params[-1], pp[-1])  # the frozen one is a copy


# ---------------------------------------------------------------- against the restatement (runs everywhere)

@pytest.mark.parametrize("kw", SCHEDULES)
def test_get_decay_matches_the_restatement(kw):
    p = EMA()(_tensors(), decay=0.9999, **kw)
    for t in DECAY_STEPS:
        assert p.get_decay(t) == ema_ref.get_decay(t, decay=0.9999, **kw), (kw, t)
    # the documented landmarks of the warmup: 0.999 at 31.6K steps
    assert abs(ema_ref.get_decay(31623, use_ema_warmup=True) - 0.999) < 1e-5 and ema_ref.get_decay(0) == 0.0 == ema_ref.get_decay(1)


@pytest.mark.parametrize("kw", [dict(decay=0.999, use_ema_warmup=True, update_after_step=1), dict(decay=0.9), dict(decay=0.0), dict(decay=1.0)])
def test_six_cpu_steps_match_the_restatement_bit_for_bit(kw):
    ps = _tensors(3)
    p = EMA()(ps, **kw)
    start = [s.numpy().copy() for s in p.shadow_params]
    sets = []
    g = torch.Generator().manual_seed(5)
    for _ in range(6):
        _nudge(ps, g)
        sets.append([t.detach().numpy().copy() for t in ps])
        p.step(ps)
    want, decay, n = ema_ref.run(start, sets, [t.requires_grad for t in ps], **kw)
    assert p.optimization_step == n == 6 and p.cur_decay_value == decay
    for i, (w, s) in enumerate(zip(want, p.shadow_params)):
        assert np.array_equal(w.view(np.uint32), s.numpy().view(np.uint32)), i


def test_contracted_form_is_a_different_function():
    """the draw the GPU test holds the kernel to: an fma in the kernel would change at least 1 % of its elements"""
    s, p = ema_ref.contraction_draw()
    a, b = ema_ref.step(s, p, 0.9999), ema_ref.step_contracted(s, p, 0.9999)
    frac = (a.view(np.uint32) != b.view(np.uint32)).mean()
    print(f"[ema] contracted form differs on {100 * frac:.2f} % of {s.size} elements")
    assert frac >= 0.01
    assert np.array_equal(ema_ref.step(s, p, 0.5, trains=False), p)


# ---------------------------------------------------------------- CPU API behaviour

def test_store_copy_to_restore_round_trip():
    ps = _tensors(1)
    e = EMA()(ps, decay=0.5)
    g = torch.Generator().manual_seed(2)
    for _ in range(6):
        _nudge(ps, g)
        e.step(ps)
    raw = [p.detach().clone() for p in ps]
    assert any(not torch.equal(s, p) for s, p in zip(e.shadow_params, ps))
    e.store(ps)
    assert all(t.device.type == "cpu" for t in e.temp_stored_params)
    e.copy_to(ps)
    for s, p in zip(e.shadow_params, ps):
        assert torch.equal(s, p.detach())
    e.restore(ps)
    assert e.temp_stored_params is None
    for r, p in zip(raw, ps):
        assert torch.equal(r, p.detach())
    with pytest.raises(RuntimeError, match="no `store\\(\\)`ed weights"):
        e.restore(ps)
    e.to(dtype=torch.float64)
    assert all(s.dtype == torch.float64 for s in e.shadow_params)
    e.step(ps)  # other dtypes take the torch path
    assert e.optimization_step == 7


def test_load_state_dict_checks_raise_the_reference_errors():
    e = EMA()(_tensors())
    good = e.state_dict()
    bad = [("decay", 1.5, "Decay must be between 0 and 1"), ("decay", -0.1, "Decay must be between 0 and 1"),
           ("min_decay", 1, "Invalid min_decay"), ("optimization_step", 1.0, "Invalid optimization_step"),
           ("update_after_step", "3", "Invalid update_after_step"), ("use_ema_warmup", 1, "Invalid use_ema_warmup"),
           ("inv_gamma", "1", "Invalid inv_gamma"), ("power", None, "Invalid power"),
           ("shadow_params", (torch.zeros(1),), "shadow_params must be a list"), ("shadow_params", [1.0], "shadow_params must all be Tensors")]
    for k, v, msg in bad:
        with pytest.raises(ValueError, match=msg):
            EMA()(_tensors()).load_state_dict(dict(good, **{k: v}))
    f = EMA()(_tensors(9))
    e.optimization_step, e.decay = 7, 0.75
    f.load_state_dict(e.state_dict())
    assert f.optimization_step == 7 and f.decay == 0.75
    for a, b in zip(e.shadow_params, f.shadow_params):
        assert torch.equal(a, b) and a.data_ptr() != b.data_ptr()  # a deep copy, like the module API


def _tiny_showo_cpu():
    d, sd_np = util.tiny_state()
    S = util.pkg().Showo
    m = S(d.w_clip_vit, d.vocab, d.llm_vocab, codebook_size=d.codebook, num_vq_tokens=d.num_vq_tokens, hidden_size=d.hidden,
          intermediate_size=d.ffn, num_hidden_layers=d.layers, num_attention_heads=d.heads)
    m.load_state_dict(util.O.to_torch(sd_np), strict=True)
    return d, m


def test_save_pretrained_writes_a_model_directory_of_the_shadows(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)  # from_pretrained's default device: this test stays on the CPU
    S = util.pkg().Showo
    d, m = _tiny_showo_cpu()
    plain = str(tmp_path / "plain")
    m.save_pretrained(plain)
    before = json.load(open(os.path.join(plain, "config.json")))
    e = EMA()(m.parameters(), decay=0.75, use_ema_warmup=True, power=0.5, model_cls=S, model_config=dict(m.config, **m.arch))
    for _ in range(3):
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(1.5)
        e.step(m.parameters())
    assert e.optimization_step == 3 and e.cur_decay_value > 0
    out = str(tmp_path / "ema")
    e.save_pretrained(out)
    cfg = json.load(open(os.path.join(out, "config.json")))
    for k in STATE_KEYS[:-1]:
        assert cfg[k] == getattr(e, k), k
    assert {k: v for k, v in cfg.items() if k not in STATE_KEYS and k != "_registered"} == before  # the model's own entries are unchanged
    m2 = S.from_pretrained(out, device="cpu")
    got = list(m2.parameters())
    assert len(got) == len(e.shadow_params)
    for s, p, q in zip(e.shadow_params, got, m.parameters()):
        assert torch.equal(s, p.detach()) and not torch.equal(p.detach(), q.detach())
    e2 = EMA().from_pretrained(out, S)
    for k in STATE_KEYS[:-1]:
        assert getattr(e2, k) == getattr(e, k), k
    for a, b in zip(e.shadow_params, e2.shadow_params):
        assert torch.equal(a, b)
    assert e2.model_cls is S and e2.get_decay(10) == e.get_decay(10)
    # a plain save of a model writes what it wrote before, and load_config's one-value form is unchanged
    assert json.load(open(os.path.join(plain, "config.json"))) == S.load_config(plain) == before
    with pytest.raises(ValueError, match="model_cls"):
        EMA()(_tensors()).save_pretrained(str(tmp_path / "x"))
    with pytest.raises(ValueError, match="model_config"):
        EMA()(_tensors(), model_cls=S).save_pretrained(str(tmp_path / "x"))


def test_trainer_takes_ema_and_rejects_bad_values_before_touching_the_device():
    T = util.pkg().Trainer
    assert inspect.signature(T.__init__).parameters["ema"].default is None
    assert callable(T.ema_weights)
    stub = types.SimpleNamespace(params=[], pparams=[], model=None)
    assert T._make_ema(stub, None) is None
    for bad in (True, "0.9", [0.9]):
        with pytest.raises(TypeError):
            T._make_ema(stub, bad)
    with pytest.raises(ValueError):
        T._make_ema(stub, 1.5)
    e = T._make_ema(stub, {"decay": 0.5, "update_after_step": 2})
    assert isinstance(e, EMA()) and e.decay == 0.5 and e.update_after_step == 2 and e.shadow_params == []


# ---------------------------------------------------------------- surface

def test_entry_points_are_declared_bound_and_exported():
    L = util.lib()
    lib = L.load()
    hdr = open(os.path.join(util.ROOT, "include", "showo_hip.h")).read()
    declared = set(re.findall(r"\b(showo_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert name in L.EXPORTED_SYMBOLS and (name in L._PROTOS or name in L._VOID) and hasattr(lib, name), name
    assert re.search(r"int showo_train_ema_swap\(showo_trainer\* t, void\* stream\);", hdr)
    assert re.search(r"int showo_train_set_ema\(showo_trainer\* t, float one_minus_decay\);", hdr)
    # the optimizer step keeps its argument list: the EMA rides on an announcement, not on a new signature
    assert re.search(r"int showo_train_adamw_step\(showo_trainer\* t, float lr, float beta1, float beta2, float eps, float weight_decay, int step,\s*void\* stream\);", hdr)
    # host-side argument checks need no GPU
    assert lib.showo_ema_table_update(None, None, 0.5, None) != 0 and b"null handle" in lib.showo_last_error()
    assert lib.showo_train_ema_swap(None, None) != 0
    assert lib.showo_train_set_ema(None, 0.5) != 0
