"""Every launcher ends in common.h:rf_launch: no other source launches a kernel or opts in to large LDS by hand, and the helpers and kernels
that rf_xcd_contiguous / rf_slice_sum replaced have no second definition."""
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
CSRC = REPO / 'retrieval-fuse_amd' / 'csrc'
SOURCES = sorted(CSRC.glob('*.hip')) + sorted(CSRC.glob('*.h')) + sorted((REPO / 'include').glob('*.h'))


def test_only_common_h_launches_and_opts_in():
    assert len(SOURCES) > 30
    for src in SOURCES:
        if src.name != 'common.h':
            for word in ('hipLaunchKernelGGL', 'RfLdsOptIn'):
                assert word not in src.read_text(), f'{src.name} names {word}: launch through rf_launch'


def test_replaced_copies_stay_gone():
    for src in SOURCES:
        for word in ('up_xcd_contiguous', 'k_wgrad_sum', 'k_wgrad_reduce(', 'k_linear_wgrad_reduce'):
            assert word not in src.read_text(), f'{src.name} names {word}'
