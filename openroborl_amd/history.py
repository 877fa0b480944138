"""The sensor history a history student reads (ppo.ActorCritic(history=16)): its dimensions and the plain-torch statement of orr_history_push.
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
