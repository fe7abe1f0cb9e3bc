"""Host (no GPU): the data models of the strategies that run on the mixed GP.  A categorical
domain without surrogate specs gets a default MixedSingleTaskGPSurrogate per output in the five
single-objective strategies, as the reference's _generate_surrogate_specs does; the others keep
their error, and the FREE categorical method refuses a mixed spec.  Mixed specs are held in
``BotorchSurrogates.mixed_surrogates``: ``surrogates`` keeps taking stationary specs only."""
import json

import pytest
from pydantic import ValidationError

import everest_amd.data_models as dm


def _domain(n_out=1):
    cont = [dm.ContinuousInput(key="x0", bounds=(0, 1)), dm.ContinuousInput(key="x1", bounds=(0, 1))]
    cats = [dm.CategoricalInput(key="c0", categories=["a", "b", "c"]),
            dm.CategoricalInput(key="c1", categories=["u", "v", "w"], allowed=[True, False, True])]
    outs = [dm.ContinuousOutput(key="y", objective=dm.MinimizeObjective(w=1.0)),
            dm.ContinuousOutput(key="z", objective=dm.MaximizeObjective(w=1.0))][:n_out]
    return dm.Domain(inputs=dm.Inputs(features=cont + cats), outputs=dm.Outputs(features=outs))


def test_sobo_on_a_categorical_domain_defaults_to_mixed_specs():
    s = dm.SoboStrategy(domain=_domain())
    specs = s.surrogate_specs.mixed_surrogates
    assert [type(m) for m in specs] == [dm.MixedSingleTaskGPSurrogate] and s.surrogate_specs.surrogates == []
    assert specs[0].outputs.get_keys() == ["y"] and specs[0].inputs.get_keys() == s.domain.inputs.get_keys()
    assert specs[0].input_preprocessing_specs == {"c0": dm.CategoricalEncodingEnum.ONE_HOT,
                                                  "c1": dm.CategoricalEncodingEnum.ONE_HOT}
    assert s.surrogate_specs.input_preprocessing_specs == specs[0].input_preprocessing_specs


@pytest.mark.parametrize("cls,n_out", [(dm.AdditiveSoboStrategy, 2), (dm.MultiplicativeSoboStrategy, 2),
                                       (dm.MultiplicativeAdditiveSoboStrategy, 2), (dm.QparegoStrategy, 2)])
def test_every_strategy_in_scope_defaults_to_mixed_specs(cls, n_out):
    s = cls(domain=_domain(n_out))
    assert [type(m) for m in s.surrogate_specs.mixed_surrogates] == [dm.MixedSingleTaskGPSurrogate] * n_out
    assert s.surrogate_specs.surrogates == []
    assert sorted(s.surrogate_specs.outputs.get_keys()) == ["y", "z"]


def test_a_continuous_domain_keeps_the_stationary_default():
    dom = _domain()
    dom = dm.Domain(inputs=dm.Inputs(features=dom.inputs.get(dm.ContinuousInput).features), outputs=dom.outputs)
    s = dm.SoboStrategy(domain=dom)
    assert [type(m) for m in s.surrogate_specs.surrogates] == [dm.SingleTaskGPSurrogate]
    assert s.surrogate_specs.mixed_surrogates == []


@pytest.mark.parametrize("cls", [dm.MoboStrategy, dm.QehviStrategy, dm.QnehviStrategy])
def test_strategies_out_of_scope_keep_their_error(cls):
    with pytest.raises(ValidationError, match="explicit SingleTaskGPSurrogate"):
        cls(domain=_domain(2))


def test_active_learning_keeps_its_error():
    with pytest.raises(ValidationError, match="explicit SingleTaskGPSurrogate"):
        dm.ActiveLearningStrategy(domain=_domain())


def test_free_refuses_a_mixed_spec():
    dom = _domain()
    with pytest.raises(ValidationError, match="FREE not compatible"):
        dm.SoboStrategy(domain=dom, categorical_method="FREE")
    spec = dm.MixedSingleTaskGPSurrogate(inputs=dom.inputs, outputs=dom.outputs)
    with pytest.raises(ValidationError, match="FREE not compatible"):
        dm.SoboStrategy(domain=dom, categorical_method="FREE", surrogate_specs=dm.BotorchSurrogates(mixed_surrogates=[spec]))
    # explicit one-hot SingleTaskGP specs stay free to use FREE
    one_hot = dm.SingleTaskGPSurrogate(inputs=dom.inputs, outputs=dom.outputs)
    s = dm.SoboStrategy(domain=dom, categorical_method="FREE", surrogate_specs=dm.BotorchSurrogates(surrogates=[one_hot]))
    assert [type(m) for m in s.surrogate_specs.surrogates] == [dm.SingleTaskGPSurrogate]
    assert s.surrogate_specs.mixed_surrogates == []


def test_mixed_specs_enter_botorch_surrogates_by_their_own_field():
    dom = _domain()
    spec = dm.MixedSingleTaskGPSurrogate(inputs=dom.inputs, outputs=dom.outputs)
    with pytest.raises(ValidationError):            # ``surrogates`` takes stationary specs only, as before
        dm.BotorchSurrogates(surrogates=[spec])
    bs = dm.BotorchSurrogates(mixed_surrogates=[spec])
    assert bs.all_surrogates == [spec] and bs.outputs.get_keys() == ["y"]
    assert bs.input_preprocessing_specs == spec.input_preprocessing_specs
    back = dm.BotorchSurrogates(**json.loads(bs.model_dump_json()))
    assert back == bs and isinstance(back.mixed_surrogates[0], dm.MixedSingleTaskGPSurrogate)
    # an explicit mixed spec for one output is kept; the other output gets the default
    s = dm.AdditiveSoboStrategy(domain=_domain(2), surrogate_specs=bs)
    assert [m.outputs.get_keys() for m in s.surrogate_specs.mixed_surrogates] == [["y"], ["z"]]
    assert s.surrogate_specs.mixed_surrogates[0] == spec


def test_json_round_trip_of_a_mixed_strategy():
    s = dm.SoboStrategy(domain=_domain(), acquisition_function=dm.qLogEI(), seed=3, num_raw_samples=64)
    back = dm.SoboStrategy(**json.loads(s.model_dump_json()))
    assert back == s
    assert [type(m) for m in back.surrogate_specs.mixed_surrogates] == [dm.MixedSingleTaskGPSurrogate]
    assert back.surrogate_specs.mixed_surrogates[0].continuous_kernel.type == "MaternKernel"


def test_strategies_out_of_scope_refuse_explicit_mixed_specs():
    """Given explicit mixed specs the data model builds; the strategy refuses them by name."""
    from everest_amd import strategies

    dom = _domain(2)
    specs = dm.BotorchSurrogates(mixed_surrogates=[
        dm.MixedSingleTaskGPSurrogate(inputs=dom.inputs, outputs=dm.Outputs(features=[f]))
        for f in dom.outputs.features])
    for cls in (dm.MoboStrategy, dm.QnehviStrategy):
        with pytest.raises(NotImplementedError, match="MixedSingleTaskGPSurrogate"):
            strategies.map(cls(domain=dom, surrogate_specs=specs))
    dom1 = _domain()
    spec1 = dm.BotorchSurrogates(mixed_surrogates=[dm.MixedSingleTaskGPSurrogate(inputs=dom1.inputs, outputs=dom1.outputs)])
    with pytest.raises(NotImplementedError, match="MixedSingleTaskGPSurrogate"):
        strategies.map(dm.ActiveLearningStrategy(domain=dom1, surrogate_specs=spec1))
