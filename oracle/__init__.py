"""oracle — CPU restatement of the reference hot path.  TEST INFRASTRUCTURE ONLY.

Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may
import anything from here, and only as the checker / the timed CPU baseline. The
product (``a2cat-vn-pytorch_amd/vnav``) never imports it and has no CPU fallback.

Pinning: the restatement is checked against golden vectors produced by running the
reference itself in the build container (``tests/golden/gen_env_goldens.py`` under the
image's Anaconda python3.9 with h5py/skimage, ``tests/golden/gen_model_goldens.py``
under python3.10 + torch) — see ``tests/test_oracle_goldens.py``. The A2C update
math lives in the absent ``deep-rl==0.2.9`` package: that part is "parity unpinned"
(see ``oracle/a2c.py`` and DESIGN.md).

Modules
  philox.py   Philox4x32-10 (the engine's counter RNG contract) in numpy
  graph.py    graph/util.py grid kernel: steps, BFS tables, h5 row builder
  envs.py     cached.py env (single), the batched VectorEnv contract, maze env
  frames.py   synthetic frame hash (scene, state, word) -> uint8 frames
  policy.py   BigGoalHouseModel trunk + heads in torch fp32 (CPU)
  a2c.py      n-step returns / A2C loss / clip / RMSprop restated in torch fp32 (CPU), and
              the float64 numpy references of the A2C step / update kernels (*64)
  a2c_cases.py  deterministic inputs of the A2C step tests (shared by the GPU tests and
              the CPU check of their draws' distance to the CDF boundaries)
  trunk_checks.py  the checks the GPU policy tests share: error measures, the activation
              store's views and ReLU masks (under goal runs read at each run's start), gradients vs
              the fp64 oracle, the recurrent core vs torch's float64 nn.LSTM
  few_env_cases.py  case tables and inputs of the few-env / float-frame / 1..7-action tests
  unreal_head_cases.py  case tables of the UNREAL head tests and the launch rules (split-K,
              weight-gradient slabs, reduce lanes, colsum blocks) that place them
  aux_head_cases.py  case tables of the aux deconv head tests, the launch rules (samples per
              item, bands, persistent grids, the finish kernel's lanes, the two-stage reduce) that
              place them, seeded inputs and the float64 restatement of the heads and their checks
  goal_trunk_cases.py  the goal trunk's launch regimes above 16 rows at the three geometries (the
              split-K / slab / lane rules of unreal_head_cases.py on its shapes, the persistent kernels'
              band structs restated), the switches in n and a smallest case list around them
  lstm_regime_cases.py  the recurrent core's launch regimes from 18 to 1030 envs (the same split-K / slab /
              lane rules on the shapes of gates, dh, dz5, dW_cat and the heads), the switches in E found
              from the launch code's inequalities, a case list covering every value of every key, the
              calling forms above 16 envs, and inputs made on the CPU (lstm_core_check(inputs=...))
  update_checks.py  one A2CTrainer update restated in float64, the UNREAL terms included
"""
