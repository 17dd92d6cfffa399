"""Host side of the set form of generation evaluation (hvgan.generation_eval.process_images_batch / evaluate_experiments over
hv_gen_eval_batch): the C ABI is declared and exported, and the wrapper's grouping, its ragged-input check and the skip-and-average rule
work without a device."""
import math
import re

import numpy as np
import pytest
import torch

import gen_eval_ref as ref


def test_batch_entries_declared_and_exported():
    from hvgan import lib
    src = open(lib.HEADER).read()
    assert re.search(r'size_t\s+hv_gen_eval_batch_workspace_bytes\s*\(int H, int W, int Z, int view, int N, int E\)\s*;', src)
    assert re.search(r'int\s+hv_gen_eval_batch\s*\(const void\* const\* ori_ct, const void\* const\* fake_ct, int ct_dtype', src)
    _, protos = lib.parse_header()
    res, args = protos['hv_gen_eval_batch']
    single = protos['hv_gen_eval'][1]
    assert len(args) == len(single) + 2 and args[0] is args[1] is lib.ctypes.c_void_p          # tables of pointers; + N, E
    assert protos['hv_gen_eval_batch_workspace_bytes'] == (lib.ctypes.c_size_t, [lib.ctypes.c_int] * 6)
    L = lib.get()
    assert hasattr(L.cdll, 'hv_gen_eval_batch') and hasattr(L.cdll, 'hv_gen_eval_batch_workspace_bytes')
    # host arithmetic of the size entry: 0 for a bad argument, growing with N and E, and the single entry's size unchanged by all this
    size = lambda *a: L.size('hv_gen_eval_batch_workspace_bytes', *a)
    assert size(37, 45, 29, 2, 0, 1) == 0 and size(37, 45, 29, 2, 1, 0) == 0 and size(37, 45, 29, 3, 1, 1) == 0
    assert 0 < size(37, 45, 29, 2, 1, 1) < size(37, 45, 29, 2, 1, 2) < size(37, 45, 29, 2, 2, 2)
    assert size(37, 45, 29, 2, 2, 2) < 2 * size(37, 45, 29, 2, 1, 2)             # the constant slack is paid once


def _vol(shape, dtype=np.float64, order='C'):
    return np.zeros(shape, dtype=dtype, order=order)


def test_grouping_by_shape_dtype_and_strides():
    from hvgan import generation_eval as GE
    A, B = (8, 9, 10), (8, 9, 11)
    originals = [(_vol(A), _vol(A, np.uint8), 20),                       # 0
                 (_vol(B), _vol(B, np.uint8), 20),                       # 1: another shape
                 (_vol(A), _vol(A, np.uint8), 21),                       # 2: as 0
                 (_vol(A, np.float32), _vol(A, np.uint8), 20),           # 3: another CT dtype
                 (_vol(A, order='F'), _vol(A, np.uint8, 'F'), 20),       # 4: other strides
                 (_vol(A), _vol(A, np.uint8), 20)]                       # 5: as 0, but one of its fakes is Fortran-ordered
    fakes = [[(_vol(o[0].shape, o[0].dtype, 'F' if o[0].flags.f_contiguous else 'C'),
               _vol(o[1].shape, o[1].dtype, 'F' if o[1].flags.f_contiguous else 'C')) for _ in range(2)] for o in originals]
    fakes[5][1] = (_vol(A, order='F'), _vol(A, np.uint8))
    E, groups = GE.group_items(originals, fakes)
    assert E == 2
    assert [idx for _, idx in groups] == [[0, 2], [1], [3], [4], [5]]
    sig = dict((tuple(idx), s) for s, idx in groups)
    assert sig[(0, 2)] == (A, torch.float64, (90, 10, 1), torch.uint8, (90, 10, 1))
    assert sig[(3,)][1] == torch.float32 and sig[(4,)][2] == (1, 8, 72)
    assert sig[(5,)][2] is None and sig[(5,)][4] == (90, 10, 1)          # mismatched CT strides inside the item: made contiguous
    # an int16 label volume is converted to float64, like process_images does
    originals[1] = (_vol(B), _vol(B, np.int16), 20)
    assert GE.group_items(originals, fakes)[1][1][0][3] == torch.float64
    # counts only: no CT
    E, groups = GE.group_items([(None, _vol(A, np.uint8), 1)], [[(None, _vol(A, np.uint8))]], counts_only=True)
    assert groups[0][0] == (A, None, None, torch.uint8, (90, 10, 1))


def test_ragged_and_mismatched_inputs_raise_before_any_device_work():
    from hvgan import generation_eval as GE
    A = (8, 9, 10)
    originals = [(_vol(A), _vol(A, np.uint8), 20) for _ in range(3)]
    pair = (_vol(A), _vol(A, np.uint8))
    with pytest.raises(ValueError, match='ragged.*item 2'):
        GE.process_images_batch(originals, [[pair, pair], [pair, pair], [pair]])
    with pytest.raises(ValueError, match='3 originals'):
        GE.process_images_batch(originals, [[pair], [pair]])
    with pytest.raises(ValueError, match='item 1'):
        GE.process_images_batch(originals, [[pair], [(_vol((8, 9, 11)), _vol(A, np.uint8))], [pair]])
    with pytest.raises(ValueError, match='view'):
        GE.process_images_batch(originals, [[pair]] * 3, view='axial')
    with pytest.raises(ValueError, match="experiment 'b' has 2 volumes"):
        GE.evaluate_experiments(originals, {'a': [pair] * 3, 'b': [pair] * 2})


def test_skip_and_average_on_a_hand_made_array():
    from hvgan import generation_eval as GE
    out = np.zeros((4, 3, 16))
    vals = np.arange(1.0, 8.0)
    for i in range(4):
        out[i, 0, :7] = vals * (i + 1)
    out[:, 1, :7] = vals
    out[0, 1, 2] = math.nan          # patch psnr NaN: skipped
    out[1, 1, 3] = 0.0               # patch ssim 0: skipped
    out[2, 1, 2] = math.inf          # kept
    # experiment 2: every volume skipped (all zeros)
    res = [GE.average_outputs(out[:, e]) for e in range(3)]
    assert res[0]['count'] == 4 and res[1]['count'] == 2 and res[2]['count'] == 0
    for q, k in enumerate(GE.KEYS):
        assert res[0][k] == float(np.mean([vals[q] * (i + 1) for i in range(4)]))
        assert math.isnan(res[2][k])
    assert res[1]['patch_psnr'] == math.inf and res[1]['iou'] == vals[4] and res[1]['global_psnr'] == vals[0]
    assert res[1]['per_volume'][1] == tuple(out[1, 1, :7]) and len(res[1]['per_volume']) == 4
    # the same rule as the restatement's
    want, n = ref.main_average([tuple(o[:7]) for o in out[:, 1]])
    assert n == 2 and all(res[1][k] == want[k] for k in GE.KEYS)
    # error flags raise, naming the volume
    out[3, 0, 7] = 1.0
    with pytest.raises(ValueError, match=r'volume 3\).*does not contain'):
        GE.average_outputs(out[:, 0])
    out[3, 0, 7], out[2, 0, 8] = 0.0, 1.0
    with pytest.raises(ValueError, match=r'my set 2:.*shorter than 7'):
        GE.average_outputs(out[:, 0], what='my set %d')
