"""Writes tests/golden/organic_mf_*.npz: the UNMODIFIED reference's OrganicMFSquare (recogym/agents/organic_mf.py) trained by the
reference's offline protocol (bench_agents.py:168-190, restated here call for call on the reference's own env and agent) under the
uniform logging policy, with the counter RNG injected into the env.

    python tests/make_golden_organic_mf.py   (needs the reference package; never imported by a test)

Each file keeps the log columns of the run (`log_*`; the two-log case a second one, `log2_*`), the agent's initial weights
(torch.manual_seed(agent_seed) directly before its construction), the reference's weights and RMSprop square averages after
training, its act per last viewed product, and the rows of a short evaluation run of the trained agent with `with_ps_all`
(`eval_*`, `eval_psa` = the index of the one in every bandit row's `ps-a`).

  organic_mf_p10_s0, organic_mf_p10_s01            P = 10, E = 5, batch 32, sigma_omega = 0 / 0.1
  organic_mf_p10_s0_org, organic_mf_p10_s01_org    the same with 25 organic-only users in front
  organic_mf_p10_mb4                               mini_batch_size = 4: steps without any pair occur (asserted)
  organic_mf_p40_e8                                P = 40, E = 8
  organic_mf_p10_two                               two logs, the boundary inside a mini-batch (asserted)

The maker records the reference's smallest top-two logit gap and REJECTS an agent seed whose gap is below 100 times
organic_mf_util.TOL_F64_VS_REFERENCE, so that the table comparison of the tests leaves out no product.  It also measures what the
tests' tolerance rests on: the largest |float64 NumPy restatement - reference weight| over the fixtures (printed)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import organic_mf_util as ou  # noqa: E402
import ref_harness as rh  # noqa: E402
from make_golden import BASE  # noqa: E402
from make_golden_logreg_poly import small  # noqa: E402

N_EVAL = 30


def reference_agent(P, E, mb, seed, with_ps_all=False):
    import torch
    from recogym import Configuration
    from recogym.agents.organic_mf import OrganicMFSquare, organic_mf_square_args
    torch.manual_seed(seed)
    return OrganicMFSquare(Configuration({**organic_mf_square_args, 'num_products': P, 'embed_dim': E, 'mini_batch_size': mb,
                                          'with_ps_all': with_ps_all}))


def weights(agent):
    ps = [agent.product_embedding.weight, agent.output_layer.weight, agent.output_layer.bias]
    w = [p.detach().numpy().astype(np.float32).copy() for p in ps]
    sq = [agent.optimizer.state[p]['square_avg'].numpy().astype(np.float32).copy() if 'square_avg' in agent.optimizer.state[p]
          else np.zeros(tuple(p.shape), np.float32) for p in ps]
    return w, sq


def offline_protocol(env, agent, n_users, n_organic):
    """bench_agents.py:168-190 -> the sessions the agent was shown, call by call."""
    seen, uid = [], 0
    for _ in range(n_organic):
        env.reset(uid)
        uid += 1
        obs, _, _, _ = env.step(None)
        seen.append([int(s['v']) for s in obs.sessions()])
        agent.train(obs, None, None, True)
    for _ in range(n_users):
        env.reset(uid)
        uid += 1
        new_obs, _, done, reward = env.step(None)
        while not done:
            old_obs = new_obs
            action, new_obs, reward, done, _ = env.step_offline(old_obs, reward, done)
            seen.append([int(s['v']) for s in old_obs.sessions()])
            agent.train(old_obs, action, reward, False)
        old_obs = new_obs
        action, _, reward, done, _ = env.step_offline(old_obs, reward, done)
        seen.append([int(s['v']) for s in old_obs.sessions()])
        agent.train(old_obs, action, reward, True)
    return seen


def one_log(args, n_users, n_organic, agent):
    """The reference's log of the run and the agent trained on the same run -> (columns, sessions shown)."""
    env = rh.make_reference_env(args)
    rh.inject_counter_rng(env, None, None)
    cols = rh.log_to_arrays(env.generate_logs(n_users, None, n_organic))
    env = rh.make_reference_env(args)
    rh.inject_counter_rng(env, None, None)
    seen = offline_protocol(env, agent, n_users, n_organic)
    assert seen == ou.walk_calls(cols['u'], cols['z'] == 1, cols['v'], n_organic), 'the log does not hold the calls of the protocol'
    return cols, seen


def run_case(name, env_over, P=10, E=5, mb=32, n_users=40, n_organic=0, second=None, seeds=range(7, 40)):
    import torch
    args = {**BASE, 'random_seed': 42, 'num_products': P, **env_over}
    for seed in seeds:
        agent = reference_agent(P, E, mb, seed, with_ps_all=True)
        w0, _ = weights(agent)
        lr = agent.optimizer.param_groups[0]['lr']
        cols, seen = one_log(args, n_users, n_organic, agent)
        logs = [(cols, seen, n_organic)]
        if second is not None:
            assert len(seen) % mb != 0, 'the boundary between the two logs must fall inside a mini-batch'
            logs.append(one_log({**args, 'random_seed': args['random_seed'] + 1}, second, 0, agent) + (0,))
        w, sq = weights(agent)
        with torch.no_grad():
            logits = agent.output_layer(agent.product_embedding(torch.arange(P))).numpy()
        top = np.sort(logits, axis=1)
        gap = float((top[:, -1] - top[:, -2]).min())
        if gap < 100 * ou.TOL_F64_VS_REFERENCE:
            print(f'{name}: agent seed {seed} rejected, top-two gap {gap:.2e}')
            continue
        break
    else:
        raise AssertionError(f'{name}: no agent seed passes the gap condition')
    # the float64 restatement on the same pairs
    model, k, pending, n_steps, n_empty = ou.NumpyModel(*w0), 0, [], 0, 0
    for _, s, _ in logs:
        steps, pending = ou.walk_steps(s, k, mb, pending)
        k += len(s)
        for pairs in steps:
            model.step(pairs, lr)
            n_steps += 1
            n_empty += len(pairs) == 0
    dev = max(float(np.abs(x - y).max()) for x, y in zip(model.arrays(), w + sq))
    assert (model.table() == logits.argmax(axis=1)).all()
    if name.endswith('mb4'):
        assert n_empty > 0, 'the mini_batch_size = 4 case needs a step without pairs'
    # a short evaluation run of the trained agent
    env = rh.make_reference_env(args)
    rh.inject_counter_rng(env, None, None)
    df = env.generate_logs(N_EVAL, agent)
    ev = rh.log_to_arrays(df)
    psa = np.array([-1 if x is None or len(x) == 0 else int(np.argmax(x)) for x in df['ps-a'].values], dtype=np.int32)
    for x in df['ps-a'].values[ev['z'] == 1]:
        assert np.sum(x) == 1.0 and np.max(x) == 1.0
    arrays = dict(small(cols, 'log_'), **small(ev, 'eval_'), eval_psa=psa, emb0=w0[0], w0=w0[1], b0=w0[2], emb=w[0], w=w[1], b=w[2],
                  sq_emb=sq[0], sq_w=sq[1], sq_b=sq[2], table=logits.argmax(axis=1).astype(np.int32))
    if second is not None:
        arrays.update(small(logs[1][0], 'log2_'))
    meta = dict(env_args=args, n_users=n_users, n_organic=n_organic, n_users2=second, n_eval=N_EVAL, agent_seed=seed, num_products=P,
                embed_dim=E, mini_batch_size=mb, learning_rate=lr, calls=k, steps=n_steps, empty_steps=n_empty, top_two_gap=gap,
                float64_deviation=dev, weight_magnitude=float(max(np.abs(x).max() for x in w)), rng='philox')
    path = os.path.join(ou.GOLDEN, name + '.npz')
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
    print(f'{name}: {len(cols["t"])} rows, {k} calls, {n_steps} steps ({n_empty} empty), gap {gap:.2e}, float64 deviation {dev:.2e}'
          f' -> {os.path.getsize(path) / 1024:.0f} KiB')
    assert os.path.getsize(path) <= 100 * 1024
    return dev


def main():
    assert rh.reference_available(), 'needs the reference package'
    rh.import_reference()
    devs = [run_case('organic_mf_p10_s0', dict(sigma_omega=0.0)),
            run_case('organic_mf_p10_s01', dict(sigma_omega=0.1)),
            run_case('organic_mf_p10_s0_org', dict(sigma_omega=0.0), n_organic=25),
            run_case('organic_mf_p10_s01_org', dict(sigma_omega=0.1), n_organic=25),
            run_case('organic_mf_p10_mb4', dict(sigma_omega=0.1), mb=4, n_users=15),
            run_case('organic_mf_p40_e8', dict(sigma_omega=0.1), P=40, E=8),
            run_case('organic_mf_p10_two', dict(sigma_omega=0.1), n_users=25, second=20)]
    print(f'largest float64 deviation from the reference: {max(devs):.3e}')


if __name__ == '__main__':
    main()
