"""The seeded configuration generators of tests/test_gpu_config_fuzz.py, shared with tests/test_gpu_physical_constants.py,
tests/fuzz_soak.py and the CPU test that holds every draw to the host's validation (tests/test_host.py).  NumPy only."""


def draw_config(rng):
    scenario = str(rng.choice(["PredatorCapturePrey", "Warehouse", "MaterialTransport", "Simple", "ArcticTransport"],
                              p=[0.35, 0.2, 0.2, 0.15, 0.1]))
    ov, n_act = {}, 5
    common = {"penalize_violations": bool(rng.rand() < 0.8), "barrier_certificate": str(rng.choice(["safe", "default"], p=[0.7, 0.3])),
              "collision_variant": str(rng.choice(["offset", "center"], p=[0.7, 0.3])), "robotarium": bool(rng.rand() < 0.15)}
    if scenario == "PredatorCapturePrey":
        n = int(rng.randint(2, 17))
        npred = int(rng.randint(1, n))
        ov = {"predator": npred, "capture": n - npred, "n_agents": n, "num_prey": int(rng.choice([1, 2, 6, 8, 9, 12, 20, 33, 35])),
              "num_neighbors": int(rng.randint(0, n + 3)), "capability_aware": bool(rng.rand() < 0.4),
              "start_dist": 0.3 if n <= 16 else 0.25, "predator_radius": float(rng.choice([0.45, 0.3, 0.7])),
              "capture_radius": float(rng.choice([0.25, 0.15, 0.4]))}
        if ov["num_prey"] > 30:
            ov["step_dist"] = 0.16                      # prey grid 5 x 11 = 55 cells
    elif scenario == "Warehouse":
        n = int(rng.randint(2, 17))
        ov = {"n_agents": n, "num_neighbors": int(rng.randint(0, n + 3)), "start_dist": 0.6 if n < 12 else 0.4,
              "goal_width": float(rng.choice([0.5, 0.3, 0.9]))}
    elif scenario == "MaterialTransport":
        n = int(rng.randint(4, 17))
        nf = int(rng.randint(0, n + 1))
        ov = {"n_agents": n, "n_fast_agents": nf, "n_slow_agents": n - nf, "start_dist": 0.3 if n <= 5 else 0.25 if n <= 13 else 0.2,
              "capability_aware": bool(rng.rand() < 0.4)}
        n_act = 20
    elif scenario == "Simple":
        ov = {"n_agents": int(rng.randint(2, 17))}
    if scenario != "ArcticTransport":
        ov.update(common)
    else:
        ov.update({k: common[k] for k in ("penalize_violations", "collision_variant")})
    if ov.get("robotarium"):
        ov["update_frequency"] = int(rng.choice([10, 17]))          # a controller every sub-step: keep the oracle affordable
    E = int(rng.choice([1, 5, 63, 64, 65, 129, 300]))
    kernel = str(rng.choice(["group", "tpe"]))
    return scenario, ov, n_act, E, kernel


def draw_config_extended(rng):
    """draw_config plus the axes the first 320 draws hold fixed: sub-steps per env step (incl. a remainder chunk of every
    length and steps shorter than a controller period), episode length (resets every few steps), step length, safety
    radius, QP sweep cap and larger ragged batches.  Used by tests/fuzz_soak.py (a one-off campaign, not part of the tier)."""
    scenario, ov, n_act, E, kernel = draw_config(rng)
    if not ov.get("robotarium"):
        ov["update_frequency"] = int(rng.choice([1, 4, 5, 11, 14, 15, 16, 29, 30, 33, 44, 61, 74]))
    ov["max_episode_steps"] = int(rng.choice([1, 2, 3, 7, 20, 80]))
    if rng.rand() < 0.3:
        ov["qp_max_sweeps"] = int(rng.choice([1, 2, 3, 5, 9]))
    if scenario in ("PredatorCapturePrey", "Warehouse", "Simple") and rng.rand() < 0.5:
        ov["step_dist"] = float(rng.choice([0.16, 0.25, 0.3])) if ov.get("num_prey", 0) <= 30 else 0.16
    if rng.rand() < 0.25:
        E = int(rng.choice([257, 1000, 2049]))
    return scenario, ov, n_act, E, kernel


def draw_barrier_family(rng):
    """draw_config plus the arguments of rps' certificate factories (config keys safety_radius, barrier_gain,
    unsafe_barrier_gain, magnitude_limit: what the reference reaches through Controller('custom', create_..._certificate2(...)),
    utilities/controller.py:11-18).  Radii above the start spacing begin inside the unsafe set (the unsafe gain at work),
    magnitude limits below the position controller's 0.15 exercise the 'threshold control inputs' branch."""
    scenario, ov, n_act, E, kernel = draw_config(rng)
    ov["safety_radius"] = float(rng.choice([0.12, 0.17, 0.2, 0.25, 0.32]))
    ov["barrier_gain"] = float(rng.choice([10.0, 100.0, 1000.0]))
    ov["unsafe_barrier_gain"] = float(rng.choice([1e4, 1e6, 1e7]))
    ov["magnitude_limit"] = float(rng.choice([0.1, 0.15, 0.2, 0.3]))
    return scenario, ov, n_act, E, kernel


def draw_interior_point(rng):
    """draw_config restricted to what `barrier_solver: cvxopt` admits (n_agents <= 8), with the certificate family and cvxopt's own
    options drawn too (tight tolerances: many iterations; a small iteration cap: the cap binds)."""
    while True:
        scenario, ov, n_act, E, kernel = draw_barrier_family(rng) if rng.rand() < 0.5 else draw_config(rng)
        n = int(ov.get("n_agents", 4))
        if n <= 8:
            break
    ov["barrier_solver"] = "cvxopt"
    if rng.rand() < 0.3:
        ov["cvxopt_reltol"] = float(rng.choice([1e-1, 1e-3, 1e-5]))
        ov["cvxopt_feastol"] = float(rng.choice([1e-1, 1e-2, 1e-4]))
    if rng.rand() < 0.2:
        ov["cvxopt_maxiters"] = int(rng.choice([0, 1, 4, 12]))
    return scenario, ov, n_act, min(E, 129), kernel
