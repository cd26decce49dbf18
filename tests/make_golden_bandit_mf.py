"""Writes tests/golden/bandit_mf_dev_*.npz: the UNMODIFIED reference's BanditMFSquare (recogym/agents/bandit_mf.py) trained by the
reference's offline protocol (bench_agents.py:168-190, restated here call for call on the reference's own env and agent) under the
uniform logging policy, with the counter RNG injected into the env.

    python tests/make_golden_bandit_mf.py   (needs the reference package; never imported by a test)

Each file keeps the log columns of the run (`log_*`; the two-log case a second one, `log2_*`), the agent's initial embeddings
(torch.manual_seed(agent_seed) directly before its construction), the reference's embeddings and RMSprop square averages after
training, its act per last viewed product (`table`) and the float32 logit it logs as `ps` there (`table_ps`).

  bandit_mf_dev_p10_s0, bandit_mf_dev_p10_s01            P = 10, E = 5, batch 32, sigma_omega = 0 / 0.1
  bandit_mf_dev_p10_s0_org, bandit_mf_dev_p10_s01_org    the same with 25 organic-only users in front
  bandit_mf_dev_p10_mb4                                  mini_batch_size = 4
  bandit_mf_dev_p40_e8                                   P = 40, E = 8
  bandit_mf_dev_p10_two                                  two logs, the boundary inside a mini-batch (asserted)

The maker records the reference's smallest top-two logit gap and REJECTS an agent seed whose gap is below 100 times
bandit_mf_util.TOL_F64_VS_REFERENCE, so that the table comparison of the tests leaves out no product.  It also measures what the
tests' tolerance rests on: the largest |float64 NumPy restatement - reference value| over the fixtures, printed at the end — the
figure that stands in bandit_mf_util.MEASURED_F64_VS_REFERENCE (run the maker again after changing it: the gap condition reads it)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import bandit_mf_util as bu  # noqa: E402
import ref_harness as rh  # noqa: E402
from make_golden import BASE  # noqa: E402
from make_golden_logreg_poly import small  # noqa: E402


def reference_agent(P, E, mb, seed):
    import torch
    from recogym import Configuration
    from recogym.agents.bandit_mf import BanditMFSquare, bandit_mf_square_args
    torch.manual_seed(seed)
    return BanditMFSquare(Configuration({**bandit_mf_square_args, 'num_products': P, 'embed_dim': E, 'mini_batch_size': mb}))


def weights(agent):
    ps = [agent.product_embedding.weight, agent.user_embedding.weight]
    w = [p.detach().numpy().astype(np.float32).copy() for p in ps]
    sq = [agent.optimizer.state[p]['square_avg'].numpy().astype(np.float32).copy() if 'square_avg' in agent.optimizer.state[p]
          else np.zeros(tuple(p.shape), np.float32) for p in ps]
    return w, sq


def offline_protocol(env, agent, n_users, n_organic):
    """bench_agents.py:168-190 -> what the agent was shown, call by call: (the session's views, action, reward)."""
    seen, uid = [], 0

    def show(obs, action, reward, done):
        seen.append(([int(s['v']) for s in obs.sessions()], None if action is None else int(action['a']),
                     None if action is None else int(reward)))
        agent.train(obs, action, reward, done)

    for _ in range(n_organic):
        env.reset(uid)
        uid += 1
        obs, _, _, _ = env.step(None)
        show(obs, None, None, True)
    for _ in range(n_users):
        env.reset(uid)
        uid += 1
        new_obs, _, done, reward = env.step(None)
        while not done:
            old_obs = new_obs
            action, new_obs, reward, done, _ = env.step_offline(old_obs, reward, done)
            show(old_obs, action, reward, False)
        old_obs = new_obs
        action, _, reward, done, _ = env.step_offline(old_obs, reward, done)
        show(old_obs, action, reward, True)
    return seen


def one_log(args, n_users, n_organic, agent):
    """The reference's log of the run and the agent trained on the same run -> (columns, calls shown)."""
    env = rh.make_reference_env(args)
    rh.inject_counter_rng(env, None, None)
    cols = rh.log_to_arrays(env.generate_logs(n_users, None, n_organic))
    env = rh.make_reference_env(args)
    rh.inject_counter_rng(env, None, None)
    seen = offline_protocol(env, agent, n_users, n_organic)
    is_b = cols['z'] == 1
    assert seen == bu.walk_calls(cols['u'], is_b, cols['v'], cols['a'], np.where(is_b, cols['c'], 0), n_organic), \
        'the log does not hold the calls of the protocol'
    return cols, seen


def run_case(name, env_over, P=10, E=5, mb=32, n_users=40, n_organic=0, second=None, seeds=range(7, 60)):
    import torch
    args = {**BASE, 'random_seed': 42, 'num_products': P, **env_over}
    for seed in seeds:
        agent = reference_agent(P, E, mb, seed)
        w0, _ = weights(agent)
        lr = agent.optimizer.param_groups[0]['lr']
        cols, seen = one_log(args, n_users, n_organic, agent)
        logs = [(cols, seen)]
        if second is not None:
            assert len(seen) % mb != 0 and len(agent.train_data[0]) > 0, 'the boundary between the two logs must fall inside a mini-batch'
            logs.append(one_log({**args, 'random_seed': args['random_seed'] + 1}, second, 0, agent))
        w, sq = weights(agent)
        with torch.no_grad():
            logits = np.stack([agent.forward(agent.all_products, np.full(P, l)).numpy() for l in range(P)])     # [last view][action]
        top = np.sort(logits, axis=1)
        gap = float((top[:, -1] - top[:, -2]).min())
        if gap < 100 * bu.TOL_F64_VS_REFERENCE:
            print(f'{name}: agent seed {seed} rejected, top-two gap {gap:.2e}')
            continue
        break
    else:
        raise AssertionError(f'{name}: no agent seed passes the gap condition')
    # the float64 restatement on the same triples
    model, k, pending, last_view, n_steps, n_empty = bu.NumpyModel(*w0), 0, [], None, 0, 0
    for _, s in logs:
        steps, pending, last_view = bu.walk_steps(s, k, mb, pending, last_view)
        k += len(s)
        for triples in steps:
            model.step(triples, lr)
            n_steps += 1
            n_empty += len(triples) == 0
    assert last_view == agent.last_product_viewed and pending == list(zip(*agent.train_data)), 'the walk is not the reference\'s train'
    dev = max(float(np.abs(x - y).max()) for x, y in zip(model.arrays(), w + sq))
    table = logits.argmax(axis=1)
    assert (model.table() == table).all()
    arrays = dict(small(cols, 'log_'), ep0=w0[0], eu0=w0[1], ep=w[0], eu=w[1], sq_ep=sq[0], sq_eu=sq[1], table=table.astype(np.int32),
                  table_ps=logits[np.arange(P), table].astype(np.float32))
    if second is not None:
        arrays.update(small(logs[1][0], 'log2_'))
    meta = dict(env_args=args, n_users=n_users, n_organic=n_organic, n_users2=second, agent_seed=seed, num_products=P, embed_dim=E,
                mini_batch_size=mb, learning_rate=lr, calls=k, steps=n_steps, empty_steps=n_empty, top_two_gap=gap,
                float64_deviation=dev, weight_magnitude=float(max(np.abs(x).max() for x in w)),
                last_product_viewed=int(agent.last_product_viewed), rng='philox')
    path = os.path.join(bu.GOLDEN, name + '.npz')
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
    print(f'{name}: {len(cols["t"])} rows, {k} calls, {n_steps} steps ({n_empty} empty), gap {gap:.2e}, float64 deviation {dev:.2e}'
          f' -> {os.path.getsize(path) / 1024:.0f} KiB')
    assert os.path.getsize(path) <= 100 * 1024
    return dev


def main():
    assert rh.reference_available(), 'needs the reference package'
    rh.import_reference()
    devs = [run_case('bandit_mf_dev_p10_s0', dict(sigma_omega=0.0)),
            run_case('bandit_mf_dev_p10_s01', dict(sigma_omega=0.1)),
            run_case('bandit_mf_dev_p10_s0_org', dict(sigma_omega=0.0), n_organic=25),
            run_case('bandit_mf_dev_p10_s01_org', dict(sigma_omega=0.1), n_organic=25),
            run_case('bandit_mf_dev_p10_mb4', dict(sigma_omega=0.1), mb=4, n_users=15),
            run_case('bandit_mf_dev_p40_e8', dict(sigma_omega=0.1), P=40, E=8),
            run_case('bandit_mf_dev_p10_two', dict(sigma_omega=0.1), n_users=25, second=20)]
    print(f'largest float64 deviation from the reference: {max(devs):.3e}')


if __name__ == '__main__':
    main()
