"""The continuous-action Phasic-Policy-Gradient cases of tests/golden/ppg_gauss.npz (policy args, trainer args, sample arguments):
the generator (tests/golden/gen_ppg_gauss.py) and the tests read them from here."""
from srl_amd.runtime import synthetic

_OBS7 = {"obs": ((7,), "f32")}

PPG_GAUSS_CASES = {
    # `fixed`: log sigma is a parameter without gradient; it must come out of the epochs unchanged
    "gfix": (dict(obs_dim=7, action_dim=3, hidden_dim=32, num_dense_layers=2, num_rnn_layers=0, popart=False, layernorm=True,
                  chunk_len=8, seed=91, continuous_action=True, std_type="fixed", init_log_std=-0.3),
             dict(popart=False, ppg_epochs=3, max_grad_norm=5.0, beta_clone=1.0, aux_value_head_weight=0.5,
                  ppg_optimizer_config=dict(lr=1e-3)),
             dict(T=16, B=6, obs_spec=_OBS7, action_dims=3, p_done=0.1, continuous_action=True)),
    # `separate_learnable` under PopArt (value_dim 2): the rows' d log sigma are column-summed into the vector's gradient
    "gsep": (dict(obs_dim=7, action_dim=3, hidden_dim=32, num_dense_layers=2, num_rnn_layers=0, popart=True, layernorm=True,
                  chunk_len=8, seed=92, value_dim=2, continuous_action=True, std_type="separate_learnable"),
             dict(popart=True, ppg_epochs=2, max_grad_norm=1.0, beta_clone=2.0, aux_value_head_weight=1.0),
             dict(T=16, B=4, obs_spec=_OBS7, action_dims=3, p_done=0.1, value_dim=2, continuous_action=True)),
    # `shared_learnable`: log sigma per row from a second head on the actor's features; one action dimension
    "gshr": (dict(obs_dim=5, action_dim=1, hidden_dim=16, num_dense_layers=2, num_rnn_layers=0, popart=False, layernorm=False,
                  chunk_len=4, seed=93, activation="tanh", continuous_action=True, std_type="shared_learnable"),
             dict(popart=False, ppg_epochs=2, beta_clone=1.0, aux_value_head_weight=1.0, ppg_optimizer_config=dict(lr=5e-4)),
             dict(T=8, B=5, obs_spec={"obs": ((5,), "f32")}, action_dims=1, p_done=0.15, continuous_action=True)),
    # GRU backbones: chunked analysis from the stored states
    "ggru": (dict(obs_dim=4, action_dim=2, hidden_dim=16, num_dense_layers=1, num_rnn_layers=1, popart=False, layernorm=True,
                  chunk_len=4, seed=94, continuous_action=True, std_type="separate_learnable"),
             dict(popart=False, ppg_epochs=2, max_grad_norm=10.0, beta_clone=1.0, aux_value_head_weight=1.0,
                  ppg_optimizer_config=dict(lr=1e-3)),
             dict(T=8, B=5, obs_spec=synthetic.CARTPOLE_OBS, action_dims=2, p_done=0.1, continuous_action=True,
                  policy_state={"actor_hx": (1, 16), "critic_hx": (1, 16)})),
}

TERM_NAMES = ("auxiliary_value_loss", "value_head_loss", "policy_distance", "loss", "grad_norm")
