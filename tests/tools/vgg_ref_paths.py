"""Test helper: pickle this package's models, the VGG nets among them, under the REFERENCE's class paths."""
import sys
import types

from ref_paths import as_reference_classes as _base


def as_reference_classes(fn):
    """ref_paths.as_reference_classes (the ResNet / DenseNet / head classes; that helper's module list is fixed) with
    ``deepards.models.vgg`` claimed around it for the classes of deepards_amd.models.vgg."""
    import deepards_amd.models.vgg as V
    refname = 'deepards.models.vgg'
    fake = types.ModuleType(refname)
    moved = [obj for obj in vars(V).values() if isinstance(obj, type) and obj.__module__ == V.__name__]
    for obj in moved:
        obj.__module__ = refname
        setattr(fake, obj.__name__, obj)
    saved = sys.modules.get(refname)
    sys.modules[refname] = fake
    try:
        return _base(fn)
    finally:
        for obj in moved:
            obj.__module__ = V.__name__
        if saved is None:
            sys.modules.pop(refname, None)
        else:
            sys.modules[refname] = saved
