"""CPU: the C ABI of MCMC densification's host side (include/fdgs.h "MCMC densification, host side", csrc/mcmc.hip) -- every symbol declared,
exported and bound, ABI still 6, the refusals with their messages, a size of 0 as a no-op."""
import os
import re

import numpy as np
import pytest

import mcmc_common as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fdgs_mcmc_philox_host", "fdgs_mcmc_weights_host", "fdgs_mcmc_sample_host", "fdgs_mcmc_relocation_host", "fdgs_mcmc_normals_host",
         "fdgs_mcmc_noise_host"]


@pytest.fixture(scope="module")
def L():
    return MC.lib()


def err(L):
    return L.fdgs_last_error().decode()


def test_symbols_are_declared_exported_and_bound(L):
    src = open(os.path.join(ROOT, "include", "fdgs.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(fdgs_[a-z0-9_]+)\s*\(", src))
    for n in NAMES:
        assert n in declared, n
        assert n in MC._lib.SYMBOLS, n
        assert hasattr(L, n), n
    assert sorted(n for n in declared if n.startswith("fdgs_mcmc_")) == sorted(NAMES)
    assert L.fdgs_abi_version() == 6 and MC._lib.ABI_VERSION == 6
    assert "#define FDGS_MCMC_MAX_RATIO 51" in src
    for name, tag in MC.TAGS.items():
        assert re.search(r"#define FDGS_MCMC_TAG_%s 0x%08Xu" % (name.upper(), tag), src), name


def test_zero_size_is_a_no_op(L):
    for fn, args in ((L.fdgs_mcmc_philox_host, (0, None, 0, 0, None)), (L.fdgs_mcmc_weights_host, (0, None, 0.005, None, None)),
                     (L.fdgs_mcmc_sample_host, (0, None, 0, 0, 0, None, None)), (L.fdgs_mcmc_relocation_host, (0, None, None, None, 0.005, None, None)),
                     (L.fdgs_mcmc_normals_host, (0, 0, 0, None)), (L.fdgs_mcmc_noise_host, (0, None, None, None, None, 1.0, 100.0, 0.005, 0, 0, None))):
        assert fn(*args) == 0
    scan, src = np.ones(4, np.uint64), np.full(3, -5, np.int32)
    assert L.fdgs_mcmc_sample_host(4, MC.p(scan), 0, 0, MC.TAGS["grow"], MC.p(src), None) == 0 and (src == -5).all()      # no draws: nothing written


def test_refusals(L):
    w = np.zeros(4, np.uint32)
    assert L.fdgs_mcmc_philox_host(1, None, 0, 0, MC.p(w)) != 0 and "NULL" in err(L)
    assert L.fdgs_mcmc_philox_host(-1, None, 0, 0, MC.p(w)) != 0 and "bad sizes" in err(L)
    assert L.fdgs_mcmc_weights_host(4, None, 0.005, MC.p(w), None) != 0 and "NULL" in err(L)
    assert L.fdgs_mcmc_weights_host(-4, None, 0.005, MC.p(w), None) != 0 and "bad sizes" in err(L)
    scan = np.zeros(4, np.uint64)
    src = np.zeros(4, np.int32)
    assert L.fdgs_mcmc_sample_host(4, MC.p(scan), 4, 0, MC.TAGS["grow"], MC.p(src), None) != 0 and "no live row" in err(L)
    assert L.fdgs_mcmc_sample_host(4, None, 4, 0, MC.TAGS["grow"], MC.p(src), None) != 0 and "NULL" in err(L)
    assert L.fdgs_mcmc_sample_host(4, MC.p(scan), -1, 0, MC.TAGS["grow"], MC.p(src), None) != 0 and "bad sizes" in err(L)
    assert L.fdgs_mcmc_relocation_host(4, None, None, None, 0.005, None, None) != 0 and "NULL" in err(L)
    assert L.fdgs_mcmc_relocation_host(-1, None, None, None, 0.005, None, None) != 0 and "bad sizes" in err(L)
    assert L.fdgs_mcmc_normals_host(4, 0, 0, None) != 0 and "NULL" in err(L)
    assert L.fdgs_mcmc_normals_host(-4, 0, 0, None) != 0 and "bad sizes" in err(L)
    assert L.fdgs_mcmc_noise_host(4, None, None, None, None, 1.0, 100.0, 0.005, 0, 0, None) != 0 and "NULL" in err(L)
    assert L.fdgs_mcmc_noise_host(-1, None, None, None, None, 1.0, 100.0, 0.005, 0, 0, None) != 0 and "bad sizes" in err(L)
