// Stand-in at the include path the reference uses: empty, the particle-measure unit reads ready-made normals
// (pcl::Normal is in ref_pcl.hpp) and estimates none.
