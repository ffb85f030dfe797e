"""The structure of the engines: one tower-neutral base (ClipEngine), the ViT and RN50 engines as sibling towers, and the
hooks a tower supplies (ClipEngine.TOWER_HOOKS).  Classes and signatures only: no GPU, no library."""
import inspect
import typing

import pytest

from fairfedmed_amd import engine, engine_rn
from fairfedmed_amd.engine import FairLoRAEngine
from fairfedmed_amd.engine_rn import RN50Engine, create_engine

TOWERS = (FairLoRAEngine, RN50Engine)


def base():
    return engine.ClipEngine


def hooks(with_default):
    return [name for name, has_default in base().TOWER_HOOKS if has_default == with_default]


def params(fn):
    return list(inspect.signature(fn).parameters.values())


def test_towers_are_siblings_under_the_base():
    assert issubclass(FairLoRAEngine, base())
    assert issubclass(RN50Engine, base())
    assert not issubclass(RN50Engine, FairLoRAEngine)
    assert not issubclass(FairLoRAEngine, RN50Engine)
    assert typing.get_type_hints(create_engine, vars(engine_rn))["return"] is base()


def test_hook_list_is_the_docstring_table():
    # one source: every hook of TOWER_HOOKS heads a row of the table in the class docstring, in its order, and no other
    # row names a method
    rows = [line.split("(")[0].strip() for line in base().__doc__.splitlines()
            if line.strip().startswith(("_", "inference()"))]
    names = [n for n, _ in base().TOWER_HOOKS]
    assert rows == names[:-1]                                    # (inference() / infer share the last row)
    assert all(callable(getattr(base(), n)) for n in names)


@pytest.mark.parametrize("tower", TOWERS, ids=lambda c: c.__name__)
def test_tower_implements_every_hook_with_the_base_signature(tower):
    for name, has_default in base().TOWER_HOOKS:
        if not has_default:
            assert name in vars(tower), f"{tower.__name__} must define {name}"
        want, got = params(getattr(base(), name)), params(getattr(tower, name))
        assert [p.name for p in got[:len(want)]] == [p.name for p in want], name
        assert [p.kind for p in got[:len(want)]] == [p.kind for p in want], name
        for extra in got[len(want):]:                            # (the ViT's ws=None)
            assert extra.default is not inspect.Parameter.empty, f"{tower.__name__}.{name}: {extra.name} has no default"
            assert extra.kind in (inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY), extra.name


def test_rn50_carries_nothing_of_the_vit_tower():
    for name in ("_init_infer", "_infer_prepare"):
        assert not hasattr(RN50Engine, name), name
    assert "_after_plan" not in vars(RN50Engine)
    assert RN50Engine._after_plan is base()._after_plan
    assert RN50Engine.infer is base().infer and RN50Engine.inference is base().inference
    assert RN50Engine.infer_ws is None
    for name, fn in inspect.getmembers(RN50Engine, inspect.isfunction):
        assert not any("_InferWorkspace" in str(a) for a in fn.__annotations__.values()), name
    # ... and the ViT engine overrides the three with its forward-only pass
    assert all(name in vars(FairLoRAEngine) for name in ("infer", "inference", "_after_plan", "_init_infer"))


def test_base_hooks_without_a_default_raise():
    eng = object.__new__(base())                                 # no __init__: no GPU is touched
    for name in hooks(with_default=False):
        args = [None] * (len(params(getattr(base(), name))) - 1)
        with pytest.raises(NotImplementedError):
            getattr(eng, name)(*args)
    assert eng._after_plan(1, 1) is None                         # the one no-op
    assert eng.infer_ws is None
    with eng.inference() as e:
        assert e is eng
