"""``simple_knn`` -- the package of the reference's second CUDA extension (sugar/gaussian_splatting/submodules/simple-knn), here
backed by libgsr_hip.so: ``from simple_knn._C import distCUDA2`` works unchanged once the root of this repository is on
``sys.path`` (``autovfx_amd.install()`` puts it first)."""
