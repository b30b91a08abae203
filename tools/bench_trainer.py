"""End-to-end rate of the device evaluate/train loop (nmmo_amd/trainer.py) on one GPU: the
reference trainer's agent_SPS (clean_pufferl.py:364-376) with the HIP stepper, HBM storage and the
small stand-in policy, plus the train side (sort, GAE, PPO epochs) per update.

Usage (GPU box): python tools/bench_trainer.py [envs] [batch_size] [updates] [--fused-heads] [--fused-loss]
                                               [--recurrent] [--fused-lstm]
(--fused-heads: the agent's action heads run as the fused HIP kernels, nmmo_amd/heads.py;
 --fused-loss: the PPO minibatch loss runs as the fused HIP kernel, nmmo_amd/ppo.py;
 --recurrent: RecurrentMaskedAgent, an LSTM between encoder and heads with one state per agent slot;
 --fused-lstm: its recurrence runs as the fused HIP kernels, nmmo_amd/lstm.py; implies --recurrent)
"""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from nmmo_amd.config import Config  # noqa: E402
from nmmo_amd.engine import NmmoEngine  # noqa: E402
from nmmo_amd.trainer import DeviceTrainer, MaskedLinearAgent, RecurrentMaskedAgent, TrainConfig  # noqa: E402


def main():
    fused = "--fused-heads" in sys.argv
    fused_loss = "--fused-loss" in sys.argv
    fused_lstm = "--fused-lstm" in sys.argv
    recurrent = fused_lstm or "--recurrent" in sys.argv
    argv = [a for a in sys.argv if not a.startswith("--")]
    envs = int(argv[1]) if len(argv) > 1 else 64
    batch = int(argv[2]) if len(argv) > 2 else 32768
    updates = int(argv[3]) if len(argv) > 3 else 3
    torch.manual_seed(1)
    cfg = Config.preset("C4", early_stop_agent_num=8)
    eng = NmmoEngine(cfg, envs, seed=1)
    eng.reset()
    if recurrent:
        agent = RecurrentMaskedAgent(cfg.TASK_EMBED_DIM, fused_heads=fused, seed=1, fused_lstm=fused_lstm).cuda()
    else:
        agent = MaskedLinearAgent(cfg.TASK_EMBED_DIM, fused_heads=fused, seed=1).cuda()
    tc = TrainConfig(batch_size=batch, total_timesteps=batch * (updates + 1), fused_loss=fused_loss)
    tr = DeviceTrainer(eng, agent, tc)
    tr.evaluate()  # warm-up (allocator, kernels)
    tr.train()
    ev, trn = [], []
    for _ in range(updates):
        ev.append(tr.evaluate())
        trn.append(tr.train())
    out = {
        "workload": f"C4 {envs} envs x 128 agents, flat obs, batch_size {batch}, {type(agent).__name__}"
                    + (", fused heads" if fused else "") + (", fused loss" if fused_loss else "")
                    + (", fused lstm" if fused_lstm else ""),
        "fused_heads": fused,
        "fused_loss": fused_loss,
        "recurrent": recurrent,
        "fused_lstm": fused_lstm,
        "agent_SPS": round(sum(e["agent_SPS"] for e in ev) / len(ev)),
        "SPS": round(sum(e["SPS"] for e in ev) / len(ev)),
        "eval_time_s": round(sum(e["eval_time"] for e in ev) / len(ev), 4),
        "train_time_s": round(sum(t["train_time"] for t in trn) / len(trn), 4),
        "train_sps": round(sum(t["train_sps"] for t in trn) / len(trn)),
        "losses": {k: trn[-1][k] for k in ("policy_loss", "value_loss", "entropy", "approx_kl")},
    }
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
