"""The rule by which the differentiable rollouts of pympc_amd/torch_layer.py put the gradient of a model matrix together from what
``rollout_adjoint`` returns (``_model_paths``), stated literally for the four forms: which names, in which order -- the order of the additions
is part of what the layer computes (tests/test_gpu_rollout_layer_bits.py holds the bits)."""
import pytest

from pympc_amd.torch_layer import _model_paths


def test_the_plain_forms_give_params_every_path():
    assert _model_paths(False, False, False) == {'Ad_traj': [], 'Ad': ['Ad'], 'Bd_traj': [], 'Bd': ['Bd']}
    assert _model_paths(False, False, True) == {'Ad_traj': [], 'Ad': ['Ad', 'Ap'], 'Bd_traj': [], 'Bd': ['Bd', 'Bp']}
    assert _model_paths(True, False, False) == {'Ad_traj': [], 'Ad': ['Ad', 'Ae'], 'Bd_traj': [], 'Bd': ['Bd', 'Be']}
    assert _model_paths(True, False, True) == {'Ad_traj': [], 'Ad': ['Ad', 'Ae', 'Ap'], 'Bd_traj': [], 'Bd': ['Bd', 'Be', 'Bp']}


def test_a_schedule_of_both_matrices_takes_the_paths_entry_by_entry():
    both = dict(given_Ad=True, given_Bd=True)
    assert _model_paths(False, True, False, **both) == {'Ad_traj': ['Ad_traj'], 'Ad': ['Ad'], 'Bd_traj': ['Bd_traj'], 'Bd': ['Bd']}
    assert _model_paths(False, True, True, **both) == {'Ad_traj': ['Ad_traj', 'Ap_traj'], 'Ad': ['Ad'], 'Bd_traj': ['Bd_traj', 'Bp_traj'], 'Bd': ['Bd']}
    assert _model_paths(True, True, False, **both) == {'Ad_traj': ['Ad_traj', 'Ae_traj'], 'Ad': ['Ad'], 'Bd_traj': ['Bd_traj', 'Be_traj'], 'Bd': ['Bd']}
    assert _model_paths(True, True, True, **both) == {'Ad_traj': ['Ad_traj', 'Ae_traj', 'Ap_traj'], 'Ad': ['Ad'],
                                                      'Bd_traj': ['Bd_traj', 'Be_traj', 'Bp_traj'], 'Bd': ['Bd']}


def test_a_matrix_the_schedule_left_alone_takes_the_unsuffixed_names_of_all_its_paths():
    ad_only = dict(given_Ad=True, given_Bd=False)
    assert _model_paths(False, True, False, **ad_only) == {'Ad_traj': ['Ad_traj'], 'Ad': ['Ad'], 'Bd_traj': [], 'Bd': ['Bd']}
    assert _model_paths(False, True, True, **ad_only) == {'Ad_traj': ['Ad_traj', 'Ap_traj'], 'Ad': ['Ad'], 'Bd_traj': [], 'Bd': ['Bd', 'Bp']}
    assert _model_paths(True, True, False, **ad_only) == {'Ad_traj': ['Ad_traj', 'Ae_traj'], 'Ad': ['Ad'], 'Bd_traj': [], 'Bd': ['Bd', 'Be']}
    assert _model_paths(True, True, True, **ad_only) == {'Ad_traj': ['Ad_traj', 'Ae_traj', 'Ap_traj'], 'Ad': ['Ad'], 'Bd_traj': [], 'Bd': ['Bd', 'Be', 'Bp']}
    assert _model_paths(True, True, True, given_Ad=False, given_Bd=True) == {'Ad_traj': [], 'Ad': ['Ad', 'Ae', 'Ap'],
                                                                             'Bd_traj': ['Bd_traj', 'Be_traj', 'Bp_traj'], 'Bd': ['Bd']}


@pytest.mark.parametrize('est', (False, True))
@pytest.mark.parametrize('follows', (False, True))
def test_without_a_schedule_what_it_gave_means_nothing(est, follows):
    assert _model_paths(est, False, follows, given_Ad=True, given_Bd=True) == _model_paths(est, False, follows)
