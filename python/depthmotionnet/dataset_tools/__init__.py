"""Drop-in package path of the reference's python/depthmotionnet/dataset_tools: the View tuple and the view tools that run on the GPU
(demon_amd/view_tools.py).  The HDF5 / sun3d file handling, adjust_intrinsics, resize_view and the VTK viewer are not provided."""
