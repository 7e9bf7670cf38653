!  qn_pairs_dev -- qn_dev's loop (the reference's test/driver2.f90:66-195 on device buffers, the library's built-in
!  separable bounded quadratic, classic entry setulb_dev) to a NEW_X return, then the curvature model as data of the
!  caller's own: the stored pairs are read back on the device (lbfgsb_qn_pairs_get), loaded into a SECOND context that
!  never runs (lbfgsb_qn_pairs_set), one more pair is pushed there (lbfgsb_qn_pairs_push), and H g is taken from both
!  contexts (lbfgsb_qn_apply): the same vector before the push.
!
!     qn_pairs_dev [n [m [iterations]]]      defaults 100000, 5, 12
!
!  Output: one "Iterate" line per iterate, then
!     QNPAIRS col = <stored pairs> theta = <theta>
!     QNPAIRS run <sum of H g> <sum of its squares>          from the context of the run
!     QNPAIRS model <sum of H g> <sum of its squares>        from the context that was handed the pairs
!     QNPAIRS stored = <1> col = <stored pairs> theta = <theta>        after the push of (s, y), y = 2 s
!     QNPAIRS pushed <sum of H g> <sum of its squares>
      program qn_pairs_dev

      use lbfgsb_module, wp => lbfgsp_wp
      use iso_c_binding
      use iso_fortran_env, only: output_unit

      implicit none

      interface
         function hipMalloc(ptr, nbytes) bind(C, name='hipMalloc') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr) :: ptr
            integer(c_size_t), value :: nbytes
            integer(c_int) :: rc
         end function hipMalloc
         function hipFree(ptr) bind(C, name='hipFree') result(rc)
            import :: c_ptr, c_int
            type(c_ptr), value :: ptr
            integer(c_int) :: rc
         end function hipFree
         function hipMemcpy(dst, src, nbytes, kind) bind(C, name='hipMemcpy') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr), value :: dst, src
            integer(c_size_t), value :: nbytes
            integer(c_int), value :: kind
            integer(c_int) :: rc
         end function hipMemcpy
         function hipMemset(dst, val, nbytes) bind(C, name='hipMemset') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr), value :: dst
            integer(c_int), value :: val
            integer(c_size_t), value :: nbytes
            integer(c_int) :: rc
         end function hipMemset
      end interface
      integer(c_int), parameter :: H2D = 1, D2H = 2

      integer               :: n, m, maxit, rc, i, col, col2, stored
      real(wp), parameter   :: factr = 0.0_wp, pgtol = 0.0_wp
      character(len=60)     :: task, csave
      character(len=32)     :: arg
      logical               :: lsave(4)
      integer               :: isave(44)
      real(wp)              :: f, dsave(29)
      real(c_double)        :: theta, theta2
      type(c_ptr)           :: ctx, model, dx, dg, dl, du, dnbd, dhv, dS, dY, ds1, dy1
      real(wp), allocatable, target :: hbuf(:)
      integer(c_int32_t), allocatable, target :: hnbd(:)
      integer(c_size_t)     :: vbytes

      n = 100000; m = 5; maxit = 12
      if (command_argument_count() >= 1) then
         call get_command_argument(1, arg); read (arg, *) n
      end if
      if (command_argument_count() >= 2) then
         call get_command_argument(2, arg); read (arg, *) m
      end if
      if (command_argument_count() >= 3) then
         call get_command_argument(3, arg); read (arg, *) maxit
      end if

      vbytes = int(n, c_size_t)*int(storage_size(1.0_wp)/8, c_size_t)
      call chk(hipMalloc(dx, vbytes), 'hipMalloc x')
      call chk(hipMalloc(dg, vbytes), 'hipMalloc g')
      call chk(hipMalloc(dl, vbytes), 'hipMalloc l')
      call chk(hipMalloc(du, vbytes), 'hipMalloc u')
      call chk(hipMalloc(dhv, vbytes), 'hipMalloc H g')
      call chk(hipMalloc(ds1, vbytes), 'hipMalloc s')
      call chk(hipMalloc(dy1, vbytes), 'hipMalloc y')
      call chk(hipMalloc(dS, vbytes*int(m, c_size_t)), 'hipMalloc S')
      call chk(hipMalloc(dY, vbytes*int(m, c_size_t)), 'hipMalloc Y')
      call chk(hipMalloc(dnbd, int(n, c_size_t)*4_c_size_t), 'hipMalloc nbd')
      call chk(hipMemset(dx, 0_c_int, vbytes), 'hipMemset x')             ! x0 = 0
      call chk(hipMemset(dg, 0_c_int, vbytes), 'hipMemset g')
      allocate (hbuf(n))
      hbuf = -1.0_wp                                                       ! l = -1
      call chk(hipMemcpy(dl, c_loc(hbuf), vbytes, H2D), 'hipMemcpy l')
      hbuf = 1.0_wp                                                        ! u = +1
      call chk(hipMemcpy(du, c_loc(hbuf), vbytes, H2D), 'hipMemcpy u')
      allocate (hnbd(n))
      do i = 1, n
         hnbd(i) = int(mod(i, 4), c_int32_t)                               ! all four bound types
      end do
      call chk(hipMemcpy(dnbd, c_loc(hnbd), int(n, c_size_t)*4_c_size_t, H2D), 'hipMemcpy nbd')
      deallocate (hnbd)

      call lbfgsb_create(ctx, n, m, 0, rc)
      if (rc == 0) call lbfgsb_create(model, n, m, 0, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_create failed: ', lbfgsb_error_message()
         error stop 1
      end if

      task = 'START'
      f = 0.0_wp
      do while (task(1:2) == 'FG' .or. task == 'NEW_X' .or. task == 'START')
         call setulb_dev(ctx, dx, dl, du, dnbd, f, dg, factr, pgtol, task, -1, csave, lsave, isave, dsave, rc)
         if (rc /= 0) then
            write (output_unit, '(2a)') ' setulb_dev failed: ', lbfgsb_error_message()
            error stop 1
         end if
         if (task(1:2) == 'FG') then
            call lbfgsb_objective(ctx, 0, dx, dg, rc, f)
            if (rc /= 0) error stop 2
         else if (task(1:5) == 'NEW_X') then
            write (output_unit, '(2(a,i5,4x),a,1p,d12.5,4x,a,1p,d12.5)') 'Iterate', isave(30), 'nfg =', isave(34), &
               'f =', f, '|proj g| =', dsave(13)
            if (isave(30) >= maxit) exit                                   ! the model of this NEW_X return
         end if
      end do

      ! the pairs of this return, device to device, and H g from the context of the run
      call lbfgsb_qn_pairs_get(ctx, m, col, theta, dS, n, dY, n, rc)
      if (rc == 0) call lbfgsb_qn_apply(ctx, LBFGSB_QN_H, 1, dg, n, dhv, n, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_qn_pairs_get / lbfgsb_qn_apply failed: ', lbfgsb_error_message()
         error stop 1
      end if
      write (output_unit, '(a,i4,a,es25.16e3)') 'QNPAIRS col =', col, ' theta =', theta
      call sums('QNPAIRS run')

      ! a second context that never runs keeps them as a model of the caller's own
      call lbfgsb_qn_pairs_set(model, col, dS, n, dY, n, theta, rc)
      if (rc == 0) call lbfgsb_qn_apply(model, LBFGSB_QN_H, 1, dg, n, dhv, n, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_qn_pairs_set / lbfgsb_qn_apply failed: ', lbfgsb_error_message()
         error stop 1
      end if
      call sums('QNPAIRS model')

      ! one more pair: s_i = 1 / (1 + mod(i, 7)), y = 2 s; theta = y'y / s'y = 2
      do i = 1, n
         hbuf(i) = 1.0_wp/real(1 + mod(i, 7), wp)
      end do
      call chk(hipMemcpy(ds1, c_loc(hbuf), vbytes, H2D), 'hipMemcpy s')
      hbuf = 2.0_wp*hbuf
      call chk(hipMemcpy(dy1, c_loc(hbuf), vbytes, H2D), 'hipMemcpy y')
      call lbfgsb_qn_pairs_push(model, ds1, dy1, 0.0_c_double, stored, rc)
      if (rc == 0) call lbfgsb_qn_pairs_get(model, 0, col2, theta2, c_null_ptr, 0, c_null_ptr, 0, rc)
      if (rc == 0) call lbfgsb_qn_apply(model, LBFGSB_QN_H, 1, dg, n, dhv, n, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_qn_pairs_push / lbfgsb_qn_apply failed: ', lbfgsb_error_message()
         error stop 1
      end if
      write (output_unit, '(a,i2,a,i4,a,es25.16e3)') 'QNPAIRS stored =', stored, ' col =', col2, ' theta =', theta2
      call sums('QNPAIRS pushed')

      call lbfgsb_destroy(model)
      call lbfgsb_destroy(ctx)
      rc = hipFree(dx); rc = hipFree(dg); rc = hipFree(dl); rc = hipFree(du); rc = hipFree(dnbd)
      rc = hipFree(dhv); rc = hipFree(dS); rc = hipFree(dY); rc = hipFree(ds1); rc = hipFree(dy1)

      contains

      subroutine sums(tag)
      character(len=*), intent(in) :: tag
      real(c_double) :: a, b
      integer :: k
      call chk(hipMemcpy(c_loc(hbuf), dhv, vbytes, D2H), 'hipMemcpy H g')
      a = 0.0_c_double; b = 0.0_c_double
      do k = 1, n
         a = a + real(hbuf(k), c_double)
         b = b + real(hbuf(k), c_double)**2
      end do
      write (output_unit, '(a,2es25.16e3)') tag, a, b
      end subroutine sums

      subroutine chk(code, what)
      integer(c_int), intent(in) :: code
      character(len=*), intent(in) :: what
      if (code /= 0) then
         write (output_unit, '(3a,i0)') ' ', what, ' failed, hipError ', code
         error stop 3
      end if
      end subroutine chk

      end program qn_pairs_dev
