"""Host side of the view-general volume inference (infer.view_geometry, infer.check_volume_inputs): the slice axis, slice count and plane
shape of both views, and the argument errors that must be raised before any GPU work.  No GPU is touched."""
import numpy as np
import pytest
import torch


def test_view_geometry_of_both_views():
    import hvgan  # noqa: F401
    from hvgan import infer
    # sagittal: `[:, :, k]`, planes [A0][A1]; coronal: `[:, k, :]`, planes [A0][A2]
    assert infer.view_geometry((256, 256, 64), 'sagittal') == (2, 64, (256, 256))
    assert infer.view_geometry((256, 64, 256), 'coronal') == (1, 64, (256, 256))
    assert infer.view_geometry((37, 29, 45), 'sagittal') == (2, 45, (37, 29))        # the sagittal view does not look at the plane's shape
    assert infer.view_geometry((37, 45, 37), 'coronal') == (1, 45, (37, 37))
    assert infer.view_geometry(torch.Size([8, 3, 8]), 'coronal') == (1, 3, (8, 8))
    assert infer.view_geometry(np.zeros((4, 5, 6)).shape, 'sagittal') == (2, 6, (4, 5))
    # the slices the geometry names are numpy's
    v = np.arange(6 * 5 * 6).reshape(6, 5, 6)
    for view, take in (('sagittal', lambda k: v[:, :, k]), ('coronal', lambda k: v[:, k, :])):
        axis, n, plane = infer.view_geometry(v.shape, view)
        assert n == v.shape[axis] and all(take(k).shape == plane and np.array_equal(take(k), np.take(v, k, axis=axis)) for k in range(n))


def test_unknown_view_is_a_value_error():
    import hvgan  # noqa: F401
    from hvgan import infer
    for view in ('axial', 'Coronal', None, 2):
        with pytest.raises(ValueError, match='view'):
            infer.view_geometry((8, 8, 8), view)
    with pytest.raises(ValueError, match='view'):
        infer.process_volumes(None, [], 'cuda:0', view='axial')
    with pytest.raises(ValueError, match='output'):
        infer.process_volumes(None, [], 'cuda:0', output='pinned')
    v = np.zeros((8, 8, 8))
    with pytest.raises(ValueError, match='view'):
        infer.process_volume(None, v, v, v, 20, 'cuda:0', view='axial')
    for shape in ((8, 8), (8, 8, 8, 8), (8, 0, 8)):
        with pytest.raises(ValueError, match='volume'):
            infer.view_geometry(shape, 'sagittal')


def test_coronal_view_needs_square_planes():
    import hvgan  # noqa: F401
    from hvgan import infer
    with pytest.raises(ValueError, match=r'\(256, 256, 64\).*\[256, 64\]'):
        infer.view_geometry((256, 256, 64), 'coronal')
    v = np.zeros((16, 4, 12))
    with pytest.raises(ValueError, match=r'\(16, 4, 12\)'):
        infer.process_volume(None, v, v, v, 20, 'cuda:0', view='coronal')      # raised before the model or the device is looked at
    assert infer.check_volume_inputs(v, v, v, 'sagittal', 'cuda:0') == (2, 12, (16, 4))


def test_device_tensor_argument_errors():
    import hvgan  # noqa: F401
    from hvgan import infer
    v = np.zeros((8, 3, 8))
    t = torch.zeros(8, 3, 8, dtype=torch.float64)
    # a tensor that is not on the pipeline's device (a CPU tensor handed to a GPU pipeline)
    for args in ((t, v, v), (v, t, v), (v, v, t)):
        with pytest.raises(ValueError, match=r'\(8, 3, 8\).*cpu.*cuda:0'):
            infer.check_volume_inputs(*args, 'coronal', 'cuda:0')
    with pytest.raises(ValueError, match='cam_data.*cpu'):
        infer.process_volume(None, v, v, t, 20, 'cuda:0', view='coronal')
    # the remaining rules do not depend on which device it is: checked against the tensors' own
    assert infer.check_volume_inputs(t, t.to(torch.uint8), t.float(), 'coronal', 'cpu') == (1, 3, (8, 8))
    nc = torch.zeros(8, 8, 3, dtype=torch.float64).transpose(1, 2)
    assert nc.shape == t.shape and not nc.is_contiguous()
    with pytest.raises(ValueError, match=r'label_data \(8, 3, 8\).*\(24, 1, 3\).*contiguous'):
        infer.check_volume_inputs(t, nc, t, 'coronal', 'cpu')
    for dt in (torch.int16, torch.int64, torch.float16):
        with pytest.raises(ValueError, match=r'ct_data \(8, 3, 8\).*dtype'):
            infer.check_volume_inputs(t.to(dt), t, t, 'coronal', 'cpu')
    with pytest.raises(ValueError, match=r'cam_data has shape \(8, 3, 7\)'):
        infer.check_volume_inputs(v, v, np.zeros((8, 3, 7)), 'coronal', 'cuda:0')
