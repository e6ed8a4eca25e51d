// Stand-in at the include path the reference uses: empty, the particle-measure unit uses nothing of pcl::VoxelGrid.
