"""Build the gfx950 HIP extension in-tree:

    PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace
"""
import glob
import os

from setuptools import setup
from torch.utils.cpp_extension import BuildExtension, CUDAExtension

os.environ.setdefault("PYTORCH_ROCM_ARCH", "gfx950")


class BuildExt(BuildExtension):
    """``depends`` makes a header edit re-enter the build, but torch's ninja
    rules record no header dependencies for .hip sources and would re-link
    the stale objects: drop the objects older than a header first."""

    def build_extension(self, ext):
        newest = max(os.path.getmtime(d) for d in ext.depends)
        for obj in glob.glob(os.path.join(self.build_temp, "**", "*.o"),
                             recursive=True):
            if os.path.getmtime(obj) < newest:
                os.remove(obj)
        super().build_extension(ext)


setup(
    name="multihop_offload_amd",
    version="0.1.0",
    packages=["multihop_offload_amd"],
    ext_modules=[
        CUDAExtension(
            name="multihop_offload_amd._hip_ops",
            sources=[
                "multihop_offload_amd/ops/hip/bindings.cpp",
                "multihop_offload_amd/ops/hip/fw.hip",
                "multihop_offload_amd/ops/hip/episode.hip",
                "multihop_offload_amd/ops/hip/queueing.hip",
                "multihop_offload_amd/ops/hip/chebconv.hip",
                "multihop_offload_amd/ops/hip/optimizer.hip",
                "multihop_offload_amd/ops/hip/chebconv_large.hip",
                "multihop_offload_amd/ops/hip/step_glue.hip",
                "multihop_offload_amd/ops/hip/timeslot.hip",
            ],
            depends=["multihop_offload_amd/ops/hip/cheb_tiles.h",
                     "multihop_offload_amd/ops/hip/queue_model.h",
                     "multihop_offload_amd/ops/hip/timeslot_phases.h",
                     "multihop_offload_amd/ops/hip/gfx950.h"],
            extra_compile_args={
                "cxx": ["-O3"],
                "nvcc": ["-O3"],
            },
        )
    ],
    cmdclass={"build_ext": BuildExt},
)
