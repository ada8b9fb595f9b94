"""Sensor configs (reference shifu/configs/sensor_config.py).  Camera sensors are rendered by a ray caster against the
collision geometry (shifu_amd/units/sensors.py, shifu_amd/render.py); RayCasterSensorConfig (no counterpart in the reference, whose
to-do list names point clouds) configures a ray-caster sensor on the same caster: a height scanner, a lidar, any pattern."""
from shifu_amd.isaacgym import gymapi

from .base_config import BaseConfig


class BaseSensorConfig(BaseConfig):
    name = "DummySensor"
    frequency = 30
    data_shape = 0


class CameraSensorConfig(BaseSensorConfig):
    name = "DummyCameraSensor"
    image_types = [gymapi.IMAGE_COLOR, gymapi.IMAGE_DEPTH, gymapi.IMAGE_SEGMENTATION, gymapi.IMAGE_OPTICAL_FLOW]
    image_normalization = False
    local_lookat_positions = None
    transform = None
    attach_local_transform = None

    def __init__(self):
        props = gymapi.CameraProperties()
        for attr in dir(self.camera_props):
            if '__' not in attr:
                setattr(props, attr, getattr(self.camera_props, attr))
        self.camera_props = props
        super().__init__()

    class camera_props:
        enable_tensors = True
        use_collision_geometry = False
        width = 256
        height = 256
        near_plane = 0.1
        far_plane = 3
        horizontal_fov = 87


class RayCasterSensorConfig(BaseSensorConfig):
    """units.RayCasterSensor: `pattern` is (origins (R, 3), dirs (R, 3)) in the sensor frame -- shifu_amd.raycast.grid_pattern,
    lidar_pattern, pinhole_pattern or any arrays.  The sensor sits at `transform` = [position, quat xyzw] in the frame of the
    state tensors, or at `attach_local_transform` in the frame of the robot's rigid body `attach_body_name`.  align: "base"
    (the rays turn with the sensor), "yaw" (with its yaw about world z only) or "world"; [min_range, max_range] in metres of
    Euclidean range; ignore_robot: the rays pass through the robot's own bodies (a scanner on the trunk must not report the
    legs)."""
    name = "DummyRayCasterSensor"
    pattern = None
    transform = None
    attach_local_transform = None
    attach_body_name = None
    align = "base"
    min_range = 0.0
    max_range = 10.0
    ignore_robot = True


class ProprioceptionSensorConfig(BaseSensorConfig):
    """units.ProprioceptionSensor (no counterpart in the reference): IMUs, joint encoders and foot contact switches with the
    imperfections a robot's own sensors have.  imu: up to 4 dicts(body=<rigid body name or index>, position=(x, y, z),
    quat=(x, y, z, w)), the mounting in the body frame; feet: "auto" (the robot's end_effector_names), or up to 8 body names /
    indices, or [].  A foot switch closes above f_on newtons and opens below f_off (None: f_on) of |f| (contact_mode "norm") or
    of f_z ("z").  velocity: "direct" (the joint velocity plus noise) or "difference" (of two measured positions).  The noise
    terms are standard deviations per read (gyro rad/s, accel m/s^2, dof_pos rad, dof_vel rad/s), *_walk the bias random
    walks' densities (per sqrt(s)), *_bias / dof_offset the half-widths of the uniform draws at a reset, resolution the
    encoder's step (0: none).  delay: reads of latency, one int or (IMUs, encoders, feet), at most max_delay <= 7; randomize()
    draws them per env.  dt: seconds between two reads (None: the env's dt); gravity None: the sim's."""
    name = "DummyProprioceptionSensor"
    imu = []
    feet = "auto"
    contact_mode = "norm"
    f_on = 1.0
    f_off = None
    velocity = "direct"
    gyro_noise = 0.0
    accel_noise = 0.0
    gyro_walk = 0.0
    accel_walk = 0.0
    gyro_bias = 0.0
    accel_bias = 0.0
    dof_pos_noise = 0.0
    dof_vel_noise = 0.0
    dof_offset = 0.0
    resolution = 0.0
    delay = 0
    max_delay = 0
    dt = None
    gravity = None
    seed = 0
    backend = "auto"
