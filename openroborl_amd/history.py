"""The sensor history a history student reads (ppo.ActorCritic(history=16)): its dimensions and the plain-torch statement of orr_history_push;
and the recurrent student's GRU over the same frame (ppo.ActorCritic(recurrent=256)): the plain-torch statement of orr_gru_forward.
ppo re-exports every name."""

# the sensor history of a history student (include/openroborl_policy.h: ORR_HISTORY_*): 16 frames of 32 words, newest first
HISTORY_STEPS, HISTORY_FRAME, HISTORY_DIM = 16, 32, 512
ENC_HIDDEN = 256


def history_frame(obs):
    """The newest reading of each sensor history inside obs [N,160] + four zeros: IMU obs[0:4], last action obs[12:24], motor angles obs[48:60]."""
    import torch
    return torch.cat((obs[:, 0:4], obs[:, 12:24], obs[:, 48:60], obs.new_zeros(obs.shape[0], 4)), dim=1)


def history_push(hist, obs, done):
    """The plain-torch statement of orr_history_push: hist [N,512] before the step (None with done None), obs [N,160] the observation after
    it, done [N] the step's flags (None: everybody starts an episode) -> the history after it, a new tensor.  Slot 0 is obs's frame; a robot
    whose episode just ended has that frame in all 16 slots; everybody else's slots move one back."""
    import torch
    frame = history_frame(obs)
    fresh = frame.repeat(1, HISTORY_STEPS)
    if done is None:
        return fresh
    shifted = torch.cat((frame, hist[:, :HISTORY_DIM - HISTORY_FRAME]), dim=1)
    return torch.where(done.to(torch.bool)[:, None], fresh, shifted)


# the recurrent student (include/openroborl_policy.h: ORR_GRU_*): a GRU of 256 units over the 32-word frame, gate order r | u | c, and a
# linear layer from its state to the 48-word privileged row
GRU_HIDDEN = 256
GRU_NAMES = ("model/gru_x", "model/gru_h", "model/gru_out")


def gru_step(p, x, start, h):
    """One step of the recurrence: x [N,32] the frame, start [N] bool (the robot's episode starts with this observation: its state is reset),
    h [N,256] the state before -> the state after.  p: the parameter dict (model/gru_x, model/gru_h)."""
    import torch
    H = GRU_HIDDEN
    hp = torch.where(start.to(torch.bool)[:, None], torch.zeros_like(h), h)
    gx = x @ p["model/gru_x/w:0"] + p["model/gru_x/b:0"]
    gh = hp @ p["model/gru_h/w:0"] + p["model/gru_h/b:0"]
    r = torch.sigmoid(gx[:, :H] + gh[:, :H])
    u = torch.sigmoid(gx[:, H:2 * H] + gh[:, H:2 * H])
    c = torch.tanh(gx[:, 2 * H:] + r * gh[:, 2 * H:])
    return (1.0 - u) * c + u * hp


def encode_seq(p, obs, starts, h0):
    """The plain-torch statement of orr_gru_forward: obs [T,N,160], starts [T,N] (starts[t] = the done flags of the step that produced obs[t]),
    h0 [N,256] -> (hid [T,N,256], z [T,N,48]), z_t = h_t Wo + bo the estimate of the privileged row.  Differentiable in p."""
    import torch
    h, hid = h0, []
    for t in range(obs.shape[0]):
        h = gru_step(p, history_frame(obs[t]), starts[t], h)
        hid.append(h)
    hid = torch.stack(hid)
    return hid, hid @ p["model/gru_out/w:0"] + p["model/gru_out/b:0"]
