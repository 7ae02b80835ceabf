"""y2_anchor_kmeans and y2_anchor_assign on the MI355X against their host functions, bit for bit (both run csrc/kmeans.h; the host function is checked
against numpy in test_kmeans_cpu.py), and dimension_cluster.cluster on CUDA data against CPU data.  Valid inputs only: hostile ones are the job of
tools/kmeans_host_check.cpp on the host."""
import numpy as np
import pytest
import torch

import _hip
import dimension_cluster
import kmeans_cases as km

pytestmark = pytest.mark.gpu
KEYS = ('means', 'iters', 'status', 'cost', 'counts')


def dev():
    return torch.device('cuda', 0)


def device(size, init, max_iter=km.MAX_ITER, conv_test=km.CONV_TEST):
    """One y2_anchor_kmeans launch on the current stream into canary-filled outputs; the outputs as numpy arrays."""
    R, K = init.shape
    s, i = torch.tensor(size).to(dev()), torch.tensor(init).to(dev())
    out = dict(means=torch.full((R, K, 2), -7.0, dtype=torch.float64, device=dev()), iters=torch.full((R,), -7, dtype=torch.int32, device=dev()),
               status=torch.full((R,), -7, dtype=torch.int32, device=dev()), cost=torch.full((R,), -7.0, dtype=torch.float64, device=dev()),
               counts=torch.full((R, K), -7, dtype=torch.int32, device=dev()))
    rc = _hip.lib().y2_anchor_kmeans(s.data_ptr(), len(size), K, i.data_ptr(), R, max_iter, conv_test, *(out[k].data_ptr() for k in KEYS), _hip.stream())
    assert rc == 0
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize('case', km.CASES, ids=km.case_id)
def test_device_equals_host(case):
    got, want = device(*km.inputs(case)), km.host_case(case)
    for k in KEYS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.parametrize('N,K', [(70000, 9), (1, 1)])
def test_assign_equals_host(N, K):
    size = km.sizes(N)
    means = km.host_case((70000, 9, 2))['means'][0][:K]
    s, m = torch.tensor(size).to(dev()), torch.tensor(means).to(dev())
    index, iou = torch.full((N,), -7, dtype=torch.int32, device=dev()), torch.full((N,), -7.0, dtype=torch.float64, device=dev())
    assert _hip.lib().y2_anchor_assign(s.data_ptr(), N, m.data_ptr(), K, index.data_ptr(), iou.data_ptr(), _hip.stream()) == 0
    want_index, want_iou = km.assign_host(size, means)
    np.testing.assert_array_equal(index.cpu().numpy(), want_index)
    np.testing.assert_array_equal(iou.cpu().numpy(), want_iou)
    # either output alone
    only = torch.full((N,), -7.0, dtype=torch.float64, device=dev())
    assert _hip.lib().y2_anchor_assign(s.data_ptr(), N, m.data_ptr(), K, None, only.data_ptr(), _hip.stream()) == 0
    np.testing.assert_array_equal(only.cpu().numpy(), want_iou)


def test_cluster_on_cuda_data_equals_cpu_data():
    size = km.sizes(1000)
    want = dimension_cluster.cluster(size, 5, repeats=12, seed=4)
    got = dimension_cluster.cluster(torch.tensor(size).to(dev()), 5, repeats=12, seed=4)
    also = dimension_cluster.cluster(size, 5, repeats=12, seed=4, device=dev())
    for res in (got, also):
        assert sorted(res) == sorted(want)
        for k in want:
            np.testing.assert_array_equal(res[k], want[k], err_msg=k)


def test_second_call_on_another_stream_returns_the_same_bytes():
    case = (1000, 5, 6)
    first = device(*km.inputs(case))
    s = torch.cuda.Stream(device=dev())
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        second = device(*km.inputs(case))
    s.synchronize()
    for k in KEYS:
        assert first[k].tobytes() == second[k].tobytes(), k
