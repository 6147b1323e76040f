"""The layout of the metric vector an A2CTrainer update returns (``step(sync=False)["raw"]``), stated
once: _update_metrics assembles the vector from it, step() decodes it by segment name. Pure Python."""


def metric_layout(unreal=False, nav_metrics=False, expert=False, geo_curriculum=False, shaping=False,
                  rp_sampling=False, novelty=False, ppo=False, ppo_kl=False):
    """{segment: (offset, width)} of the vector under these trainer flags, in the vector's order
    (its width: the last segment's offset + width). fp64 with ``shaping``, whose distance sums
    are exact there, fp32 otherwise."""
    segments = (
        # value loss, action loss, entropy, return mean, grad norm, aux loss, episodes, return sum,
        # length sum; with the UNREAL losses + pc loss, rp loss, vr loss (vn_a2c_metrics_ex)
        ("base", 12 if unreal else 9, True),
        ("nav", 4, nav_metrics),  # episodes, successes, SPL sum, start-distance sum
        ("expert", 4, expert),  # sum of -log q, agreeing samples, labelled samples, the weight used
        ("curriculum", 1, geo_curriculum),  # this rank's mean level over scenes
        ("shaping", 3, shaping),  # distance-before sum, distance-after sum, the anneal's step count
        # the skewed reward-prediction draw (vn_unreal_rp_sample's stats4): zero-reward candidates,
        # non-zero ones, draws with a non-zero reward, non-void draws
        ("rp_sampling", 4, rp_sampling),
        # the novelty bonus (vn_a2c_novelty_rewards' stats4 and vn_visit_stats): the sum of the
        # added terms, the rollout's first visits, this rank's states with a count > 0
        ("novelty", 3, novelty),
        # the final PPO epoch (vn_ppo_loss_grad's ppo_stats4), sums over the N samples: the k3
        # estimate of KL(old || new), samples with |r - 1| > clip, the ratio, value-clipped samples
        ("ppo", 4, ppo),
        # the target-KL stop (vn_ppo_kl_gate's gate_dev and kl_dev): ppo_steps = the optimiser steps
        # the update was allowed, kl_stopped = 1 when a check fired, kl_at_stop = the KL that fired it
        # (0 when none did). With ppo_kl_host_stop the epochs end at the stop, so the "ppo" sums are
        # then those of the last epoch that ran, not of the final one.
        ("ppo_kl", 3, ppo_kl),
    )
    layout, offset = {}, 0
    for name, width, on in segments:
        if on:
            layout[name] = (offset, width)
            offset += width
    return layout
