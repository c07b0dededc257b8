"""Mutation check of the HOST mirror (energybalancemodel.jl_amd/*.py) against the CPU suite: python tests/tools/mutants.py run host
Each mutant is one textual change in a temporary copy of the tree, and the suite runs inside the copy.  One line per mutant:
KILLED by <first failing test> or SURVIVED (then the -m gpu suite is the next line of defence)."""
KIND = "tree"
TESTS = ("tests", "-m", "not gpu", "-x")
LIMIT = 300
MUTANTS = [
    ("winter_index_truncated", "self.winter = Collection(t=winter, inx=int(round(self.nt * winter)))", "self.winter = Collection(t=winter, inx=int(self.nt * winter))",
     "infrastructure.py"),
    ("time_axis_at_step_starts", "self.t = np.array([float(Fraction(2 * i + 1, 2 * self.nt)) for i in range(self.nt)])",
     "self.t = np.array([float(Fraction(2 * i, 2 * self.nt)) for i in range(self.nt)])", "infrastructure.py"),
    ("sin_grid_to_the_other_pole", "urange = (0.0, math.pi / 2.0)", "urange = (0.0, math.pi)", "infrastructure.py"),
    ("forcing_warming_time_from_cooling_rate", "warming = (peak - base) / rates[0]", "warming = (peak - base) / -rates[1]", "infrastructure.py"),
    ("forcing_ramp_ignores_its_start", "return self.base + self.rates[0] * (T - d[1])", "return self.base + self.rates[0] * T", "infrastructure.py"),
    ("forcing_cooling_from_base", "return self.peak + self.rates[1] * (T - d[3])", "return self.base + self.rates[1] * (T - d[3])", "infrastructure.py"),
    ("classic_time_index_without_the_half_step", "y = (t + dt / 2.0) * nt", "y = t * nt", "infrastructure.py"),
    ("shards_overlap_by_one", "return slice(start, start + base + (1 if rank < extra else 0))", "return slice(start, start + base + 1)", "ensemble.py"),
    ("shards_ignore_the_remainder", "start = rank * base + min(rank, extra)", "start = rank * base", "ensemble.py"),
]
