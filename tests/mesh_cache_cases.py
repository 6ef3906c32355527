"""The sequences of tests/test_gpu_mesh_cache.py: the generator of tests/lifecycle_cases.py as it is (the roomy variant A,
PINHOLE semantics), cut off after MAX_STEPS steps.  tests/test_changes_ref_cpu.py shows on the shadow model alone, with the rule
of tests/changes_ref.py, that each sequence has steps that list fewer blocks than the model holds."""
import lifecycle_cases as LC

VARIANT, SEM = "A", 1
SEEDS = [0, 3]
MAX_STEPS = 29                       # then one vh_remove_components: 30 steps


def changing_steps(seq):
    """(index, step) of the first MAX_STEPS steps; the caller skips readers and options as it sees fit."""
    for n, step in enumerate(seq.steps()):
        if n >= MAX_STEPS:
            break
        yield n, step


def changes_model(step):
    return step["op"] in LC.CHANGING
