"""Score a policy on an engine without the experience store: forward, step, add up the rewards.

    eng = NmmoEngine(cfg, n_envs, seed=seed)      # flat obs
    eng.reset()
    out = run_policy(eng, agent, 1024)            # greedy: the same actions on every run
    out["reward_sum"]                             # float32 [n_envs * P]

What the reference's `evaluate.py` does with a loaded checkpoint, on the device: `DeviceTrainer`'s
recv -> forward -> send loop (trainer.py) with nothing stored. The agent is called as the trainer calls
it, `agent(obs)` or, if it has an `.lstm`, `agent(obs, state)`; `greedy=True` is passed on as a keyword,
which `BaselineAgent` and `RecurrentBaselineAgent` take (the heads then select instead of sampling,
SPEC.md §24), and with `greedy=False` no keyword is passed, so any agent of trainer.py works.
"""

from __future__ import annotations

import torch


def run_policy(engine, agent, n_steps: int, *, greedy: bool = True, state=None, on_step=None) -> dict:
    """`n_steps` ticks of every env of `engine` (flat obs, already reset) under `agent`, in one
    `torch.no_grad()` loop over the engine's bound rows.

    state: a recurrent agent's (h, c), each [num_layers, n_rows, hidden], carried on from an earlier
        call; None starts from zeros. As in the trainer it is not reset when an agent dies.
    on_step(obs, actions, logprob, value): optional, for checkers; sees each step's rows [n_rows,
        obs_elems] and the agent's outputs before the engine overwrites the rows.
    Returns {"reward_sum": float32 [n_rows], each step's rewards added in step order, "agent_steps":
    the live agent rows that acted, "steps": n_steps, "state": the final LSTM state or None}, after
    `engine.check_fault`."""
    N = engine.n_envs * engine.P
    dev = engine.device
    recurrent = hasattr(agent, "lstm")
    if recurrent and state is None:
        shape = (agent.lstm.num_layers, N, agent.lstm.hidden_size)
        state = (torch.zeros(shape, device=dev), torch.zeros(shape, device=dev))
    kw = {"greedy": True} if greedy else {}
    reward_sum = torch.zeros(N, dtype=torch.float32, device=dev)
    agent_steps = torch.zeros((), dtype=torch.int64, device=dev)
    with torch.no_grad():
        for _ in range(int(n_steps)):
            o = engine.obs.view(N, engine.obs_elems)
            if recurrent:
                actions, logprob, _, value, state = agent(o, state, **kw)
            else:
                actions, logprob, _, value = agent(o, **kw)
            agent_steps += engine.mask.view(N).sum()
            if on_step is not None:
                on_step(o, actions, logprob, value.flatten())
            engine.step(actions.to(torch.int32).view(engine.n_envs, engine.P, -1))
            reward_sum += engine.rew.view(N)
    engine.check_fault("run_policy")
    return {"reward_sum": reward_sum, "agent_steps": int(agent_steps.item()), "steps": int(n_steps),
            "state": state if recurrent else None}
